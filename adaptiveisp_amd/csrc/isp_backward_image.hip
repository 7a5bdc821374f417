// Image gradients of the ISP filters for gfx950:
//   grad_img[b][c][y][x] = sum_{c',y',x'} grad_out[b][c'][y'][x'] * gate * d f_c'(y',x') / d img[b][c][y][x]
// where f is the selected filter's `process` and gate the pass-through mask of the output clip (ADAISP_CLIP01). The
// derivatives follow the reference's autograd, subgradient conventions included: clamp / clip pass the gradient on the
// closed interval [lo, hi]; max / min over the channels route it to the first channel on ties; the hue of SaturationPlus
// carries the gradient of the last masked write only; floor passes zero, % passes it unchanged; relu at 0 passes zero.
//
// Three kernel families, one launch each (two for NLM), dispatched per image on the device-side op id like
// launch_backward_params. Every output element is written by exactly one family, so nothing is accumulated and no
// atomics are needed: each family gathers the transposed stencil of its filter.
//   pointwise (E, G, W, CCM, T, C, Ct, S+, BW, and zeros for op -1 / unknown ids): per pixel, 16-byte accesses per plane;
//   stencils (Shr, ShrV2, USM): the image tile + halo in LDS, the gated output gradient of the tile + halo next to it,
//                              then the transposed 3x3 / 5x5 taps (reflect padding folded back for USM);
//   NLM (11x11 search, 5x5 patch): pass 1 recomputes the forward per pixel and writes a = g/W, b = -sum_c g_c N_c / W^2
//                              to the workspace; pass 2 walks the 121 offsets over an LDS tile and gathers the colour and
//                              patch-distance terms (see k_nlm_dimg).
#include "isp_filter_math.h"

namespace adaisp {
namespace {

constexpr int kThreads = 256;

__device__ __forceinline__ float sgn(float v) { return v > 0.0f ? 1.0f : (v < 0.0f ? -1.0f : 0.0f); }

// ---- pointwise ops -----------------------------------------------------------------------------------------------------
struct PwConst {
    float c0;           // exposure gain
    float m[3][3];      // CCM rows divided by their sums
    float tsc[3];       // 8 / sum of the curve (tone: same for the three channels)
};

__device__ __forceinline__ PwConst pw_const(int op, const float* __restrict__ p) {
    PwConst k{};
    if (op == ADAISP_OP_EXPOSURE) k.c0 = expf(p[0] * 0.6931471805599453f);
    if (op == ADAISP_OP_CCM) {
        float rs[3];
        ccm_rows(p, k.m, rs);
    }
    // The output gate of a pixel whose curve value lands on 1.0 depends on the last ulp of the curve's total, so the totals
    // are added in the order of the reference's reduction: running (tone, [B,8] contiguous: as the forward kernel) and, for
    // the colour curves' strided [B,8,3] sum, four partial sums p[i] + p[i+4] folded in order (known difference: the forward
    // and the parameter gradient add each colour curve's total as one running sum).
    if (op == ADAISP_OP_TONE) {
        float s = 0.f;
        for (int i = 0; i < 8; ++i) s += p[i];
        k.tsc[0] = k.tsc[1] = k.tsc[2] = 8.0f / (s + 1e-30f);
    }
    if (op == ADAISP_OP_COLOR)
        for (int ch = 0; ch < 3; ++ch) {
            float s = p[ch] + p[12 + ch];
            for (int i = 1; i < 4; ++i) s += p[3 * i + ch] + p[3 * (i + 4) + ch];
            k.tsc[ch] = 8.0f / (s + 1e-30f);
        }
    return k;
}

// d/d(r,g,b) of SaturationPlus (filters.py:536-560) on the clamped pixel xc, contracted with gg (already clip-gated)
__device__ void satplus_grad(const float (&x)[3], const float (&gg)[3], float a, float (&dx)[3]) {
    const float xc[3] = {clamp01(x[0]), clamp01(x[1]), clamp01(x[2])};
    const float r = xc[0], g = xc[1], b = xc[2];
    // torch.max / min over dim 1 pick the first channel on ties
    const int imx = (r >= g && r >= b) ? 0 : (g >= b ? 1 : 2);
    const int imn = (r <= g && r <= b) ? 0 : (g <= b ? 1 : 2);
    const float mx = xc[imx], mn = xc[imn];
    const float d = (mx - mn) + 1e-8f;
    // hue: sequential masked overwrites, the last writer wins (filters.py:455-466)
    int hb = -1;                                     // 0: R branch, 1: G, 2: B, 3: grey (zero)
    float hue = 0.0f;
    if (b == mx) { hue = 4.0f + (r - g) / d; hb = 2; }
    if (g == mx) { hue = 2.0f + (b - r) / d; hb = 1; }
    if (r == mx) { hue = py_mod((g - b) / d, 6.0f); hb = 0; }
    if (mn == mx) { hue = 0.0f; hb = 3; }
    hue = hue / 6.0f;
    const bool s_zero = mx == 0.0f;
    const float s = s_zero ? 0.0f : (mx - mn) / (mx + 1e-8f);
    const float kv = 0.5f - fabsf(0.5f - mx);
    const float es = s + (1.0f - s) * kv * 0.8f;
    const float h = py_mod(hue, 1.0f), s2 = clamp01(es), v2 = clamp01(mx);
    const float h6 = h * 6.0f, hi = floorf(h6), f = h6 - hi;
    // hsv2rgb (filters.py:481-533): which of v, t, p, q each channel takes
    float dv2 = 0.f, dpp = 0.f, dqq = 0.f, dtt = 0.f;
    const float d0 = gg[0] * a, d1 = gg[1] * a, d2 = gg[2] * a;
    if (hi == 0.0f) { dv2 += d0; dtt += d1; dpp += d2; }
    else if (hi == 1.0f) { dqq += d0; dv2 += d1; dpp += d2; }
    else if (hi == 2.0f) { dpp += d0; dv2 += d1; dtt += d2; }
    else if (hi == 3.0f) { dpp += d0; dqq += d1; dv2 += d2; }
    else if (hi == 4.0f) { dtt += d0; dpp += d1; dv2 += d2; }
    else if (hi == 5.0f) { dv2 += d0; dpp += d1; dqq += d2; }
    float ds2 = 0.f, df = 0.f;
    dv2 += dpp * (1.0f - s2) + dqq * (1.0f - f * s2) + dtt * (1.0f - (1.0f - f) * s2);
    ds2 += -dpp * v2 - dqq * v2 * f - dtt * v2 * (1.0f - f);
    df += -dqq * v2 * s2 + dtt * v2 * s2;
    const float dhue = (df * 6.0f) / 6.0f;           // f = 6h - floor(6h); h = hue6 % 1 (passes); hue6 = hue / 6
    const float des = ds2 * in01(es);
    float dmx = dv2 * in01(mx);
    const float ds = des * (1.0f - kv * 0.8f);
    dmx += des * (1.0f - s) * 0.8f * sgn(0.5f - mx);
    float dmn = 0.0f, dd = 0.0f;
    float dc[3] = {0.f, 0.f, 0.f};
    if (!s_zero) {
        const float den = mx + 1e-8f;
        dmx += ds * (1.0f / den - (mx - mn) / (den * den));
        dmn -= ds / den;
    }
    if (hb == 0) { const float u = dhue / d; dc[1] += u; dc[2] -= u; dd -= dhue * (g - b) / (d * d); }
    else if (hb == 1) { const float u = dhue / d; dc[2] += u; dc[0] -= u; dd -= dhue * (b - r) / (d * d); }
    else if (hb == 2) { const float u = dhue / d; dc[0] += u; dc[1] -= u; dd -= dhue * (r - g) / (d * d); }
    dmx += dd;
    dmn -= dd;
    dc[imx] += dmx;
    dc[imn] += dmn;
#pragma unroll
    for (int c = 0; c < 3; ++c) dx[c] = (gg[c] * (1.0f - a) + dc[c]) * in01(x[c]);
}

template <int OP>
__device__ __forceinline__ void pw_grad(const float (&x)[3], const float (&go)[3], const float* __restrict__ p,
                                        const PwConst& k, bool clip, float (&dx)[3]) {
    if (OP == ADAISP_OP_EXPOSURE) {
#pragma unroll
        for (int c = 0; c < 3; ++c) dx[c] = go[c] * gate01(x[c] * k.c0, clip) * k.c0;
    } else if (OP == ADAISP_OP_GAMMA) {
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            // m^p on the hardware log2 / exp2 (~1 ulp each: the gradient, not the forward's bit pattern; a known difference from
            // the forward's pow_pos and the parameter gradient's powf), m^(p-1) = m^p / m
            const float m = fmaxf(x[c], 0.001f);
            const float f = __builtin_amdgcn_exp2f(p[0] * __builtin_amdgcn_logf(m));
            dx[c] = x[c] >= 0.001f ? go[c] * gate01(f, clip) * (p[0] * f / m) : 0.0f;
        }
    } else if (OP == ADAISP_OP_WB) {
#pragma unroll
        for (int c = 0; c < 3; ++c) dx[c] = go[c] * gate01(x[c] * p[c], clip) * p[c];
    } else if (OP == ADAISP_OP_CCM) {
        float gg[3];
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            const float f = (x[0] * k.m[c][0] + x[1] * k.m[c][1]) + x[2] * k.m[c][2];
            gg[c] = go[c] * gate01(f, clip);
        }
#pragma unroll
        for (int j = 0; j < 3; ++j) dx[j] = (gg[0] * k.m[0][j] + gg[1] * k.m[1][j]) + gg[2] * k.m[2][j];
    } else if (OP == ADAISP_OP_TONE || OP == ADAISP_OP_COLOR) {
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            float acc = 0.0f, slope = 0.0f;
#pragma unroll
            for (int j = 0; j < 8; ++j) {
                const float t = x[c] - 0.125f * (float)j;
                const float pj = p[OP == ADAISP_OP_TONE ? j : 3 * j + c];
                acc += fminf(fmaxf(t, 0.0f), 0.125f) * pj;
                if (t >= 0.0f && t <= 0.125f) slope += pj;       // closed interval: a breakpoint takes both segments
            }
            dx[c] = go[c] * gate01(acc * k.tsc[c], clip) * (slope * k.tsc[c]);
        }
    } else if (OP == ADAISP_OP_CONTRAST) {
        const float L0 = lum_27_67_06(x[0], x[1], x[2]);
        const float L = clamp01(L0);
        const float cl = -cosf(3.14159274101257324f * L) * 0.5f + 0.5f, den = L + 1e-6f;
        const float a = p[0];
        float gL = 0.0f;
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            const float t1 = x[c] / den, ci = t1 * cl, f = (1.0f - a) * x[c] + a * ci;
            const float gg = go[c] * gate01(f, clip);
            const float gci = gg * a, gt1 = gci * cl;
            dx[c] = gg * (1.0f - a) + gt1 / den;
            gL += -gt1 * x[c] / (den * den) + gci * t1 * (0.5f * 3.14159274101257324f * sinf(3.14159274101257324f * L));
        }
        gL *= in01(L0);
        dx[0] += gL * 0.27f;
        dx[1] += gL * 0.67f;
        dx[2] += gL * 0.06f;
    } else if (OP == ADAISP_OP_WNB) {
        const float L = lum_27_67_06(x[0], x[1], x[2]);
        const float a = p[0];
        float gs = 0.0f, gg[3];
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            gg[c] = go[c] * gate01((1.0f - a) * x[c] + a * L, clip);
            gs += gg[c];
        }
        dx[0] = gg[0] * (1.0f - a) + a * gs * 0.27f;
        dx[1] = gg[1] * (1.0f - a) + a * gs * 0.67f;
        dx[2] = gg[2] * (1.0f - a) + a * gs * 0.06f;
    } else if (OP == ADAISP_OP_SATPLUS) {
        float gg[3] = {go[0], go[1], go[2]};
        if (clip) {
            const float xc[3] = {clamp01(x[0]), clamp01(x[1]), clamp01(x[2])};
            float fc[3];
            satplus_full(xc[0], xc[1], xc[2], fc[0], fc[1], fc[2]);     // the forward value, for the output gate
#pragma unroll
            for (int c = 0; c < 3; ++c) gg[c] *= in01(xc[c] * (1.0f - p[0]) + fc[c] * p[0]);
        }
        satplus_grad(x, gg, p[0], dx);
    } else {                                   // op -1 and ids outside enum adaisp_op: the forward wrote zeros
        dx[0] = dx[1] = dx[2] = 0.0f;
    }
}

template <int OP, bool VEC>
__device__ void dimg_pointwise(const float* __restrict__ in, const float* __restrict__ go, const float* __restrict__ p,
                               float* __restrict__ gi, long plane, bool clip) {
    const PwConst k = pw_const(OP, p);
    const long stride = (long)gridDim.x * kThreads;
    if (VEC) {
        const long nq = plane >> 2;
        for (long q = (long)blockIdx.x * kThreads + threadIdx.x; q < nq; q += stride) {
            float4 xv[3], gv[3], dv[3];
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                if (OP != ADAISP_OP_ZERO) xv[c] = ld4(reinterpret_cast<const float4*>(in + c * plane) + q);
                if (OP != ADAISP_OP_ZERO) gv[c] = ld4(reinterpret_cast<const float4*>(go + c * plane) + q);
            }
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                float x[3], g[3], d[3];
#pragma unroll
                for (int c = 0; c < 3; ++c) {
                    x[c] = OP == ADAISP_OP_ZERO ? 0.0f : reinterpret_cast<const float*>(&xv[c])[e];
                    g[c] = OP == ADAISP_OP_ZERO ? 0.0f : reinterpret_cast<const float*>(&gv[c])[e];
                }
                pw_grad<OP>(x, g, p, k, clip, d);
#pragma unroll
                for (int c = 0; c < 3; ++c) reinterpret_cast<float*>(&dv[c])[e] = d[c];
            }
#pragma unroll
            for (int c = 0; c < 3; ++c) st4(reinterpret_cast<float4*>(gi + c * plane) + q, dv[c]);
        }
    } else {
        for (long i = (long)blockIdx.x * kThreads + threadIdx.x; i < plane; i += stride) {
            float x[3], g[3], d[3];
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                x[c] = OP == ADAISP_OP_ZERO ? 0.0f : in[i + c * plane];
                g[c] = OP == ADAISP_OP_ZERO ? 0.0f : go[i + c * plane];
            }
            pw_grad<OP>(x, g, p, k, clip, d);
#pragma unroll
            for (int c = 0; c < 3; ++c) gi[i + c * plane] = d[c];
        }
    }
}

template <bool VEC>
__global__ __launch_bounds__(kThreads) void k_dimg_pointwise(const float* __restrict__ img, const float* __restrict__ go,
                                                             const int32_t* __restrict__ ids, const float* __restrict__ params,
                                                             int pstride, float* __restrict__ gimg, long plane, unsigned flags) {
    const int b = blockIdx.y;
    const long o = (long)b * 3 * plane;
    const float* p = params + (long)b * pstride;
    const bool clip = (flags & ADAISP_CLIP01) != 0;
    const int op = ids[b];
    if (op_is_conv(op) || op == ADAISP_OP_NLM) return;       // written by their own families
    switch (op) {
#define CASE(OPC) case OPC: dimg_pointwise<OPC, VEC>(img + o, go + o, p, gimg + o, plane, clip); break;
        CASE(ADAISP_OP_EXPOSURE) CASE(ADAISP_OP_GAMMA) CASE(ADAISP_OP_WB) CASE(ADAISP_OP_CCM) CASE(ADAISP_OP_TONE)
        CASE(ADAISP_OP_COLOR) CASE(ADAISP_OP_CONTRAST) CASE(ADAISP_OP_WNB) CASE(ADAISP_OP_SATPLUS)
#undef CASE
        default: dimg_pointwise<ADAISP_OP_ZERO, VEC>(img + o, go + o, p, gimg + o, plane, clip); break;
    }
}

// ---- 3x3 sharpen pair and 5x5 unsharp mask -----------------------------------------------------------------------------
// A 256-thread workgroup owns a 16 x 64 tile of one image, the three planes one after the other. Per plane:
//   xs: the image at tile +- 2R (USM: reflect-padded coordinates, the forward's padding; 3x3: zero outside the image);
//   gs: the gated output gradient at tile +- R, zero outside the image (and, for the 3x3 pair, the forward value of the
//       frame is the image itself, so the frame's gate is computed from it);
// then the transposed stencil. USM's reflect padding makes the taps of rows / columns 1, 2, H-3, H-2 fold back: their
// gradient also gathers around the mirrored coordinates (-q, 2n-2-q).
constexpr int CTH = 16, CTW = 64;

template <int R>
__device__ void dimg_conv_tile(const float* __restrict__ in, const float* __restrict__ go, const float* __restrict__ p,
                               float* __restrict__ gi, int op, int H, int W, float* __restrict__ xs, float* __restrict__ gs) {
    constexpr int XR = CTH + 4 * R, XC = CTW + 4 * R;        // image tile +- 2R
    constexpr int GR = CTH + 2 * R, GC = CTW + 2 * R;        // gradient tile +- R
    const int tid = threadIdx.x;
    const int x0 = blockIdx.x * CTW, y0 = blockIdx.y * CTH;
    const long plane = (long)H * W;

    float w[2 * R + 1][2 * R + 1];
    const float amount = stencil_weights<R>(p, w);

    for (int c = 0; c < 3; ++c) {
        const float* src = in + c * plane;
        const float* gsrc = go + c * plane;
        // (the previous plane's gather reads gs only; the barrier after these xs writes orders the gs rewrite behind it)
        for (int q = tid; q < XR * XC; q += kThreads) {
            const int ly = q / XC, lx = q - ly * XC;
            int gy = y0 - 2 * R + ly, gx = x0 - 2 * R + lx;
            float v = 0.0f;
            if (R == 2) {
                // only coordinates inside the reflect range [-2, n+1] are ever read by a pixel of the image
                if (gy >= -2 && gy <= H + 1 && gx >= -2 && gx <= W + 1) v = src[(long)reflect(gy, H) * W + reflect(gx, W)];
            } else if (gy >= 0 && gy < H && gx >= 0 && gx < W) {
                v = src[(long)gy * W + gx];
            }
            xs[q] = v;
        }
        __syncthreads();
        for (int q = tid; q < GR * GC; q += kThreads) {
            const int ly = q / GC, lx = q - ly * GC;
            const int gy = y0 - R + ly, gx = x0 - R + lx;
            float g = 0.0f;
            if (gy >= 0 && gy < H && gx >= 0 && gx < W) {
                const float* v = xs + ly * XC + lx;                 // top-left tap; the centre is xs[(ly + R, lx + R)]
                const float ctr = v[R * XC + R];
                float blur = 0.0f;
#pragma unroll
                for (int i = 0; i < 2 * R + 1; ++i)
#pragma unroll
                    for (int j = 0; j < 2 * R + 1; ++j) blur = fmaf(w[i][j], v[i * XC + j], blur);
                if (R == 1 && (gy == 0 || gy == H - 1 || gx == 0 || gx == W - 1)) blur = ctr;
                const float r = (op == ADAISP_OP_SHARPEN) ? ctr * amount + blur * (1.0f - amount) : ctr + (ctr - blur) * amount;
                g = gsrc[(long)gy * W + gx] * in01(r);      // the filter's own clamp; ADAISP_CLIP01 passes all of [0,1]
            }
            gs[q] = g;
        }
        __syncthreads();
        // gradient of the stencil output at global (gy, gx); zero outside the image (never outside gs for in-image reads)
        auto G = [&](int gy, int gx) -> float {
            if (gy < 0 || gy >= H || gx < 0 || gx >= W) return 0.0f;
            return gs[(gy - y0 + R) * GC + (gx - x0 + R)];
        };
        const int tx = tid & 63;
        for (int ty = tid >> 6; ty < CTH; ty += kThreads / 64) {
            const int gy = y0 + ty, gx = x0 + tx;
            if (gy >= H || gx >= W) continue;
            const float gq = G(gy, gx);
            float res;
            // away from the border every tap is an interior pixel of the image (no frame, no reflection): read gs directly,
            // in the same tap order as the general path below
            const bool inner = gy >= 2 * R && gy < H - 2 * R && gx >= 2 * R && gx < W - 2 * R;
            if (inner) {
                const float* gp = gs + (gy - y0 + R) * GC + (gx - x0 + R);
                float t = 0.0f;
                if (R == 1) {
#pragma unroll
                    for (int i = -1; i <= 1; ++i)
#pragma unroll
                        for (int j = -1; j <= 1; ++j) t = fmaf(w[1 - i][1 - j], gp[i * GC + j], t);
                    res = op == ADAISP_OP_SHARPEN ? gq * amount + t * (1.0f - amount) : gq * (1.0f + amount) - t * amount;
                } else {
#pragma unroll
                    for (int i = 0; i < 5; ++i)
#pragma unroll
                        for (int j = 0; j < 5; ++j) t = fmaf(w[i][j], gp[(2 - i) * GC + (2 - j)], t);
                    res = gq * (1.0f + amount) - t * amount;
                }
            } else if (R == 1) {
                // blur taps of the interior pixels around q (the frame's blur is the pixel itself)
                float t = 0.0f;
#pragma unroll
                for (int i = -1; i <= 1; ++i)
#pragma unroll
                    for (int j = -1; j <= 1; ++j) {
                        const int py = gy + i, px = gx + j;
                        if (py > 0 && py < H - 1 && px > 0 && px < W - 1) t = fmaf(w[1 - i][1 - j], G(py, px), t);
                    }
                const bool frame = gy == 0 || gy == H - 1 || gx == 0 || gx == W - 1;
                if (op == ADAISP_OP_SHARPEN) res = (frame ? gq : gq * amount) + t * (1.0f - amount);
                else res = (frame ? gq : gq * (1.0f + amount)) - t * amount;
            } else {
                // virtual (reflect-padded) coordinates that map onto q
                int vy[3], vx[3], ny = 1, nx = 1;
                vy[0] = gy; vx[0] = gx;
                if (gy >= 1 && gy <= 2) vy[ny++] = -gy;
                if (gy >= H - 3 && gy <= H - 2 && 2 * H - 2 - gy != gy) vy[ny++] = 2 * H - 2 - gy;
                if (gx >= 1 && gx <= 2) vx[nx++] = -gx;
                if (gx >= W - 3 && gx <= W - 2 && 2 * W - 2 - gx != gx) vx[nx++] = 2 * W - 2 - gx;
                float t = 0.0f;
                for (int a = 0; a < ny; ++a)
                    for (int bq = 0; bq < nx; ++bq)
#pragma unroll
                        for (int i = 0; i < 5; ++i)
#pragma unroll
                            for (int j = 0; j < 5; ++j) t = fmaf(w[i][j], G(vy[a] + 2 - i, vx[bq] + 2 - j), t);
                res = gq * (1.0f + amount) - t * amount;
            }
            gi[c * plane + (long)gy * W + gx] = res;
        }
    }
}

__global__ __launch_bounds__(kThreads) void k_dimg_conv(const float* __restrict__ img, const float* __restrict__ go,
                                                        const int32_t* __restrict__ ids, const float* __restrict__ params,
                                                        int pstride, float* __restrict__ gimg, int H, int W) {
    __shared__ float xs[(CTH + 8) * (CTW + 8)];
    __shared__ float gs[(CTH + 4) * (CTW + 4)];
    const int b = blockIdx.z;
    const int op = ids[b];
    if (!op_is_conv(op)) return;
    const long o = (long)b * 3 * H * W;
    const float* p = params + (long)b * pstride;
    if (op == ADAISP_OP_USM) dimg_conv_tile<2>(img + o, go + o, p, gimg + o, op, H, W, xs, gs);
    else dimg_conv_tile<1>(img + o, go + o, p, gimg + o, op, H, W, xs, gs);
}

// ---- NLM (11x11 search, 5x5 patch) -------------------------------------------------------------------------------------
// Notation (c = clip(x), y = lum(c), s = (sy, sx) the roll shift, so the shifted tensors read p - s):
//   D_s(p) = sum_u (y(p+u) - y(p+u-s))^2,  w_s = exp(-sqrt(relu(D_s)) / h'),  h' = relu(h) + 1e-8,
//   N(p) = sum_s w_s(p) c(p-s),  W(p) = sum_s w_s(p),  out = clamp(N / W).
// With g the gated output gradient, a = g / W and b = -sum_c g_c N_c / W^2:
//   dw_s(p) = a(p).c(p-s) + b(p);  dD_s = dw_s w_s (-1 / (2 h' sqrt D_s)) where D_s > 0, else 0 (relu at 0);
//   dt_s = Box5(dD_s);  dy(q) = sum_s 2 (y(q) - y(q-s)) dt_s(q) - 2 (y(q+s) - y(q)) dt_s(q+s);
//   dc(q) = sum_s w_s(q+s) a(q+s) + lum' dy(q);  dx = [0 <= x <= 1] dc.
// All coordinates wrap (torch.roll).
constexpr int NSR = 5, NPR = 2;
constexpr int NTH = 16, NTW = 64;

// pass 1: a (3 planes) and b per pixel into ws[b][4][H][W]. Lane = one column x 4 rows of a 16 x 64 tile; the patch
// distances are column sums of row sums, all in registers.
__global__ __launch_bounds__(kThreads) void k_nlm_ab(const float* __restrict__ img, const float* __restrict__ go,
                                                     const int32_t* __restrict__ ids, const float* __restrict__ params,
                                                     int pstride, float* __restrict__ ws, int H, int W) {
    constexpr int HY = NSR + NPR;                  // 7
    constexpr int YR = NTH + 2 * HY, YC = NTW + 2 * HY;
    constexpr int CR = NTH + 2 * NSR, CC = NTW + 2 * NSR;
    constexpr int RPT = 4;
    __shared__ float ylds[YR * YC];
    __shared__ float clds[3][CR * CC];
    const int b = blockIdx.z;
    if (ids[b] != ADAISP_OP_NLM) return;
    const long plane = (long)H * W;
    const float* in = img + (long)b * 3 * plane;
    const int x0 = blockIdx.x * NTW, y0 = blockIdx.y * NTH, tid = threadIdx.x;
    for (int q = tid; q < YR * YC; q += kThreads) {
        const int ly = q / YC, lx = q - ly * YC;
        const long g = (long)wrap(y0 + ly - HY, H) * W + wrap(x0 + lx - HY, W);
        const float r = clamp01(in[g]), gg = clamp01(in[g + plane]), bb = clamp01(in[g + 2 * plane]);
        ylds[q] = nlm_luma(r, gg, bb);
        const int cy = ly - NPR, cx = lx - NPR;
        if (cy >= 0 && cy < CR && cx >= 0 && cx < CC) {
            clds[0][cy * CC + cx] = r;
            clds[1][cy * CC + cx] = gg;
            clds[2][cy * CC + cx] = bb;
        }
    }
    __syncthreads();
    const float hh = fmaxf(params[(long)b * pstride], 0.0f) + 1e-8f;
    const float nc = -1.44269504088896341f / hh;      // exp(-dist / hh) = exp2(dist * nc), as the forward kernel
    const int tx = tid & 63, rb = (tid >> 6) * RPT;
    float num[3][RPT], den[RPT];
#pragma unroll
    for (int r = 0; r < RPT; ++r) num[0][r] = num[1][r] = num[2][r] = den[r] = 0.0f;
    for (int sx = -NSR; sx <= NSR; ++sx)
        for (int sy = -NSR; sy <= NSR; ++sy) {
            float hs[RPT + 2 * NPR];
#pragma unroll
            for (int k = 0; k < RPT + 2 * NPR; ++k) {
                const int ry = rb + k - NPR + HY;            // LDS row of pixel row rb + k - 2
                float a = 0.0f;
#pragma unroll
                for (int u = -NPR; u <= NPR; ++u) {
                    const float d = ylds[ry * YC + tx + u + HY] - ylds[(ry - sy) * YC + tx + u - sx + HY];
                    a += d * d;
                }
                hs[k] = a;
            }
#pragma unroll
            for (int r = 0; r < RPT; ++r) {
                const float D = (((hs[r] + hs[r + 1]) + hs[r + 2]) + hs[r + 3]) + hs[r + 4];
                const float wgt = __builtin_amdgcn_exp2f(__builtin_amdgcn_sqrtf(fmaxf(D, 0.0f)) * nc);
                const int ci = (rb + r + NSR - sy) * CC + tx + NSR - sx;
                num[0][r] += wgt * clds[0][ci];
                num[1][r] += wgt * clds[1][ci];
                num[2][r] += wgt * clds[2][ci];
                den[r] += wgt;
            }
        }
    const int gx = x0 + tx;
    if (gx >= W) return;
    const float* g = go + (long)b * 3 * plane;
    float* o = ws + (long)b * 4 * plane;
#pragma unroll
    for (int r = 0; r < RPT; ++r) {
        const int gy = y0 + rb + r;
        if (gy >= H) continue;
        const long i = (long)gy * W + gx;
        float bsum = 0.0f;
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            const float oc = num[c][r] / den[r];
            // clamp(N/W, 0, 1) on the closed interval (ADAISP_CLIP01 passes all of [0,1])
            const float gc = g[i + c * plane] * in01(oc);
            o[i + c * plane] = gc / den[r];
            bsum += gc * num[c][r];
        }
        o[i + 3 * plane] = -bsum / (den[r] * den[r]);
    }
}

// pass 2: 256 threads, one 16 x 32 output tile (2 outputs per lane). LDS (dynamic, 80 KB: two workgroups per CU),
// coordinates relative to the tile origin:
//   Y  y       rows -14..TH+13, cols -14..TW+13      C  c (3)   rows -12..TH+11, cols -12..TW+11
//   AB a, b    rows  -7..TH+6,  cols  -7..TW+6       HS         rows  -9..TH+8,  cols  -7..TW+6   row sums of (dy)^2
//   WS, DD     rows  -7..TH+6,  cols  -7..TW+6       HD         rows  -7..TH+6,  cols  -5..TW+4   row sums of dD
// Per offset s: HS -> (D, w, dD) -> HD -> every output gathers dt_s(q), dt_s(q+s) (column sums of HD) and w_s a at q+s.
constexpr int kNT2 = 256;
constexpr int N2H = 16, N2W = 32;
constexpr int YO = 14, YRS = N2H + 2 * YO, YCS = N2W + 2 * YO;
constexpr int CO = 12, CRS = N2H + 2 * CO, CCS = N2W + 2 * CO;
constexpr int AO = 7, ARS = N2H + 2 * AO, ACS = N2W + 2 * AO;
constexpr int HSO = 9, HSR = N2H + 2 * HSO;             // HS: cols like AB
constexpr int HDO = 5, HDC = N2W + 2 * HDO;             // HD: rows like AB
constexpr int kNlm2Floats = YRS * YCS + 3 * CRS * CCS + 4 * ARS * ACS + HSR * ACS + 2 * ARS * ACS + ARS * HDC;
constexpr size_t kNlm2Bytes = sizeof(float) * kNlm2Floats;

// f(q, row, col) for every item q of a ROWS x COLS region, the lane's items kNT2 apart (row / col stepped, no division)
template <int ROWS, int COLS, class F>
__device__ __forceinline__ void for_region(F&& f) {
    constexpr int DR = kNT2 / COLS, DC = kNT2 % COLS;
    int r = threadIdx.x / COLS, c = threadIdx.x % COLS;
    for (int q = threadIdx.x; q < ROWS * COLS; q += kNT2) {
        f(q, r, c);
        r += DR;
        c += DC;
        if (c >= COLS) { c -= COLS; ++r; }
    }
}

__global__ __launch_bounds__(kNT2) void k_nlm_dimg(const float* __restrict__ img, const int32_t* __restrict__ ids,
                                                   const float* __restrict__ params, int pstride,
                                                   const float* __restrict__ ws, float* __restrict__ gimg, int H, int W) {
    extern __shared__ __attribute__((aligned(16))) float nlm2[];
    float* Y = nlm2;
    float* C = Y + YRS * YCS;
    float* AB = C + 3 * CRS * CCS;
    float* HS = AB + 4 * ARS * ACS;
    float* WS = HS + HSR * ACS;
    float* DD = WS + ARS * ACS;
    float* HD = DD + ARS * ACS;
    const int b = blockIdx.z;
    if (ids[b] != ADAISP_OP_NLM) return;
    const long plane = (long)H * W;
    const float* in = img + (long)b * 3 * plane;
    const float* ab = ws + (long)b * 4 * plane;
    const int x0 = blockIdx.x * N2W, y0 = blockIdx.y * N2H, tid = threadIdx.x;

    for_region<YRS, YCS>([&](int q, int ly, int lx) {
        const long g = (long)wrap(y0 + ly - YO, H) * W + wrap(x0 + lx - YO, W);
        const float r = clamp01(in[g]), gg = clamp01(in[g + plane]), bb = clamp01(in[g + 2 * plane]);
        Y[q] = nlm_luma(r, gg, bb);
        const int cy = ly - (YO - CO), cx = lx - (YO - CO);
        if (cy >= 0 && cy < CRS && cx >= 0 && cx < CCS) {
            C[cy * CCS + cx] = r;
            C[CRS * CCS + cy * CCS + cx] = gg;
            C[2 * CRS * CCS + cy * CCS + cx] = bb;
        }
    });
    for_region<ARS, ACS>([&](int q, int ly, int lx) {
        const long g = (long)wrap(y0 + ly - AO, H) * W + wrap(x0 + lx - AO, W);
#pragma unroll
        for (int k = 0; k < 4; ++k) AB[k * ARS * ACS + q] = ab[g + k * plane];
    });
    const float hh = fmaxf(params[(long)b * pstride], 0.0f) + 1e-8f;
    const float nc = -1.44269504088896341f / hh, k2 = -0.5f / hh;
    auto y_at = [&](int r, int c) { return Y[(r + YO) * YCS + c + YO]; };
    const int tx = tid & (N2W - 1), ty0 = tid / N2W;       // outputs (ty0, tx) and (ty0 + 8, tx)
    float dyacc[2] = {0.f, 0.f}, dc[2][3] = {{0.f, 0.f, 0.f}, {0.f, 0.f, 0.f}};
    __syncthreads();

    for (int sx = -NSR; sx <= NSR; ++sx)
        for (int sy = -NSR; sy <= NSR; ++sy) {
            for_region<HSR, ACS>([&](int q, int lr, int lc) {           // HS: rows -9.., cols -7..
                const int r = lr - HSO, c = lc - AO;
                float a = 0.0f;
#pragma unroll
                for (int u = -NPR; u <= NPR; ++u) {
                    const float d = y_at(r, c + u) - y_at(r - sy, c + u - sx);
                    a += d * d;
                }
                HS[q] = a;
            });
            __syncthreads();
            for_region<ARS, ACS>([&](int q, int lr, int lc) {           // D, w, dD at rows -7.., cols -7..
                const int r = lr - AO, c = lc - AO;
                const float* hs = HS + (lr + HSO - AO - NPR) * ACS + lc;
                const float D = (((hs[0] + hs[ACS]) + hs[2 * ACS]) + hs[3 * ACS]) + hs[4 * ACS];
                const float dist = __builtin_amdgcn_sqrtf(fmaxf(D, 0.0f));
                const float wgt = __builtin_amdgcn_exp2f(dist * nc);
                const int ci = (r - sy + CO) * CCS + (c - sx + CO);
                const float dw = ((AB[q] * C[ci] + AB[ARS * ACS + q] * C[CRS * CCS + ci]) + AB[2 * ARS * ACS + q] * C[2 * CRS * CCS + ci])
                                 + AB[3 * ARS * ACS + q];
                WS[q] = wgt;
                DD[q] = D > 0.0f ? dw * wgt * k2 * __builtin_amdgcn_rsqf(D) : 0.0f;
            });
            __syncthreads();
            for_region<ARS, HDC>([&](int q, int lr, int lc) {           // HD: rows -7.., cols -5..
                const float* dd = DD + lr * ACS + lc + (AO - HDO) - NPR;
                HD[q] = (((dd[0] + dd[1]) + dd[2]) + dd[3]) + dd[4];
            });
            __syncthreads();
#pragma unroll
            for (int k = 0; k < 2; ++k) {
                const int r = ty0 + 8 * k, c = tx;
                const float* hq = HD + (r + AO - NPR) * HDC + c + HDO;
                const float* hp = HD + (r + sy + AO - NPR) * HDC + c + sx + HDO;
                const float dtq = (((hq[0] + hq[HDC]) + hq[2 * HDC]) + hq[3 * HDC]) + hq[4 * HDC];
                const float dtp = (((hp[0] + hp[HDC]) + hp[2 * HDC]) + hp[3 * HDC]) + hp[4 * HDC];
                const float yq = y_at(r, c);
                dyacc[k] += 2.0f * (yq - y_at(r - sy, c - sx)) * dtq - 2.0f * (y_at(r + sy, c + sx) - yq) * dtp;
                const int ai = (r + sy + AO) * ACS + c + sx + AO;
                const float wp = WS[ai];
#pragma unroll
                for (int ch = 0; ch < 3; ++ch) dc[k][ch] += wp * AB[ch * ARS * ACS + ai];
            }
            // the next offset's HS writes are read by nobody here; the barrier after them orders the WS / DD / HD rewrites
        }

    const int gx = x0 + tx;
    if (gx >= W) return;
    float* o = gimg + (long)b * 3 * plane;
#pragma unroll
    for (int k = 0; k < 2; ++k) {
        const int gy = y0 + ty0 + 8 * k;
        if (gy >= H) continue;
        const long i = (long)gy * W + gx;
#pragma unroll
        for (int ch = 0; ch < 3; ++ch) o[i + ch * plane] = in01(in[i + ch * plane]) * (dc[k][ch] + kNlmLuma[ch] * dyacc[k]);
    }
}

}  // namespace

size_t backward_image_workspace_floats(int B, int H, int W) { return (size_t)B * 4 * H * W; }

hipError_t launch_backward_image(const float* img, const float* grad_out, const int32_t* ids, const float* params,
                                 int pstride, float* grad_img, float* workspace, int B, int H, int W, unsigned flags,
                                 hipStream_t s) {
    const long plane = (long)H * W;
    const bool vec = (plane & 3) == 0 && ((reinterpret_cast<uintptr_t>(img) | reinterpret_cast<uintptr_t>(grad_out) |
                                           reinterpret_cast<uintptr_t>(grad_img)) & 15) == 0;
    long bx = ((vec ? plane / 4 : plane) + kThreads - 1) / kThreads;
    if (bx > 1024) bx = 1024;
    if (bx < 1) bx = 1;
    if (vec)
        hipLaunchKernelGGL(k_dimg_pointwise<true>, dim3((unsigned)bx, B), dim3(kThreads), 0, s, img, grad_out, ids, params,
                           pstride, grad_img, plane, flags);
    else
        hipLaunchKernelGGL(k_dimg_pointwise<false>, dim3((unsigned)bx, B), dim3(kThreads), 0, s, img, grad_out, ids, params,
                           pstride, grad_img, plane, flags);
    hipLaunchKernelGGL(k_dimg_conv, dim3((W + CTW - 1) / CTW, (H + CTH - 1) / CTH, B), dim3(kThreads), 0, s, img, grad_out,
                       ids, params, pstride, grad_img, H, W);
    const dim3 ng((W + NTW - 1) / NTW, (H + NTH - 1) / NTH, B);
    hipLaunchKernelGGL(k_nlm_ab, ng, dim3(kThreads), 0, s, img, grad_out, ids, params, pstride, workspace, H, W);
    static bool configured = false;          // dynamic LDS above the 64 KB default (idempotent)
    if (!configured) {
        hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(k_nlm_dimg),
                                           hipFuncAttributeMaxDynamicSharedMemorySize, (int)kNlm2Bytes);
        if (e != hipSuccess) return e;
        configured = true;
    }
    hipLaunchKernelGGL(k_nlm_dimg, dim3((W + N2W - 1) / N2W, (H + N2H - 1) / N2H, B), dim3(kNT2), kNlm2Bytes, s, img, ids,
                       params, pstride, workspace, grad_img, H, W);
    return hipGetLastError();
}

}  // namespace adaisp
