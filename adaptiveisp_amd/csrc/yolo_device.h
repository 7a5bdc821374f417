// Device-side helpers of libadayolo.so's kernels, once: vector types, bf16 conversions, the LDS-DMA / wait / barrier wrappers
// and the epilogue math. Kernel files include this; yolo_internal.h stays the host / launcher interface (yolo_api.hip sees
// only that). Everything is __forceinline__: a kernel file that uses none of a helper carries none of it.
#pragma once
#include "yolo_internal.h"

namespace adayolo {

typedef __attribute__((ext_vector_type(8))) __bf16 bf16x8;
typedef __attribute__((ext_vector_type(2))) __bf16 bf16x2;
typedef __attribute__((ext_vector_type(2))) float f32x2;
typedef __attribute__((ext_vector_type(4))) float f32x4;
typedef __attribute__((ext_vector_type(16))) float f32x16;
typedef __attribute__((ext_vector_type(2))) unsigned int u32x2;
typedef __attribute__((ext_vector_type(4))) unsigned int u32x4;
typedef __attribute__((ext_vector_type(4))) short s16x4;
typedef __attribute__((address_space(3))) void* lds_ptr_t;
typedef const __attribute__((address_space(1))) void* gbl_ptr_t;

// ---- bf16 <-> fp32 ------------------------------------------------------------------------------------------------------
__device__ __forceinline__ float bf16_to_f32(unsigned short h) { return __uint_as_float(((unsigned)h) << 16); }
__device__ __forceinline__ float lo_f(unsigned v) { return __uint_as_float(v << 16); }              // the two halves of a packed pair
__device__ __forceinline__ float hi_f(unsigned v) { return __uint_as_float(v & 0xFFFF0000u); }
// round-to-nearest-even pair conversion on the hardware unit (v_cvt_pk_bf16_f32) instead of ~8 integer VALU ops
__device__ __forceinline__ unsigned pack_bf16x2(float lo, float hi) {
    return __builtin_bit_cast(unsigned, __builtin_convertvector(f32x2{lo, hi}, bf16x2));
}
// the same rounding in integer arithmetic, for a lone value (no NaN case: yolo_loss.hip's to_bf has one)
__device__ __forceinline__ unsigned short f32_to_bf16(float f) {
    unsigned u = __float_as_uint(f);
    u += 0x7FFFu + ((u >> 16) & 1u);
    return (unsigned short)(u >> 16);
}

// ---- workgroup order, LDS-DMA, waits and barriers -------------------------------------------------------------------------
// block b runs on XCD b % 8: renumber so that consecutive tile ids share an XCD (and its L2)
__device__ __forceinline__ int xcd_remap(int bid, int nwg) {
    const int q = nwg >> 3, r = nwg & 7, xcd = bid & 7, idx = bid >> 3;
    return (xcd < r ? xcd * (q + 1) : r * (q + 1) + (xcd - r) * q) + idx;
}
// the zero page: 16 bytes an LDS-DMA piece reads where its tile row has nothing to fetch (rows beyond M, taps in the padding,
// k-tiles beyond K). Internal linkage: one copy per translation unit that uses it, none elsewhere
[[maybe_unused]] static __device__ __attribute__((aligned(16))) unsigned int g_zero16[4] = {0u, 0u, 0u, 0u};
// branch-free choice between a tensor address and the zero page
__device__ __forceinline__ unsigned long long sel(bool ok, unsigned long long p, unsigned long long z) {
    const unsigned long long m = ok ? ~0ull : 0ull;
    return (p & m) | (z & ~m);
}
// 16 bytes per lane from global memory straight into LDS (global_load_lds_dwordx4)
__device__ __forceinline__ void dma16(unsigned long long gaddr, void* l) {
    __builtin_amdgcn_global_load_lds((gbl_ptr_t)gaddr, (lds_ptr_t)l, 16, 0, 0);
}
__device__ __forceinline__ void dma16(const void* g, void* l) {
    __builtin_amdgcn_global_load_lds((gbl_ptr_t)g, (lds_ptr_t)l, 16, 0, 0);
}
template <int N>
__device__ __forceinline__ void wait_vm() {
    asm volatile("s_waitcnt vmcnt(%0)" ::"n"(N) : "memory");
}
template <int N>
__device__ __forceinline__ void wait_vm_and_barrier() {
    asm volatile("s_waitcnt vmcnt(%0)\n\ts_barrier" ::"n"(N) : "memory");
}
// s_barrier alone, fenced against the scheduler: for kernels that place their own counted waits in front of it
__device__ __forceinline__ void barrier() {
    __builtin_amdgcn_sched_barrier(0);
    asm volatile("s_barrier" ::: "memory");
    __builtin_amdgcn_sched_barrier(0);
}
// ... behind lgkmcnt(0): this wave's LDS writes are complete before the others read them (kernels that exchange data through
// plain ds_write, with no wait of their own)
__device__ __forceinline__ void barrier_lgkm() {
    __builtin_amdgcn_sched_barrier(0);
    asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory");
    __builtin_amdgcn_sched_barrier(0);
}

// buffer descriptor of a whole tensor (32-bit offsets): words 2 and 3, and the offset that is out of range for it — a load
// there returns zeros, an LDS-DMA writes zeros
constexpr unsigned kOOB = 0xFFFFFFFFu;
constexpr unsigned kRecords = 0xFFFFFF00u;
constexpr unsigned kDescFlags = 0x00020000u;
// bytes per pixel row of a wave's epilogue region in LDS: 64 channels of bf16 + 16 bytes of pad (conflict-free ds_read_b128)
constexpr int kEpiPitch = 144;

// ---- implicit-GEMM row addressing ---------------------------------------------------------------------------------------
// output pixel m -> (image, row, column) by multiply-high (ConvArgs::magic_*): the two runtime divisions cost ~80 VALU each
__device__ __forceinline__ void pixel_split(const ConvArgs& a, int m, int& b, int& ho, int& wo) {
    b = a.sh_hw < 0 ? m : (int)(__umulhi((unsigned)m, a.magic_hw) >> a.sh_hw);
    const int rem = m - b * (a.Ho * a.Wo);
    ho = a.sh_w < 0 ? rem : (int)(__umulhi((unsigned)rem, a.magic_w) >> a.sh_w);
    wo = rem - ho * a.Wo;
}
// ... and the input pixel (hi0, wi0) its window starts at (negative in the padding)
__device__ __forceinline__ void window_origin(const ConvArgs& a, int m, int& b, int& hi0, int& wi0) {
    int ho, wo;
    pixel_split(a, m, b, ho, wo);
    hi0 = ho * a.stride - a.pad; wi0 = wo * a.stride - a.pad;
}
// bit tap = kh * ks + kw: that tap of the window lies inside the image. Validity is separable: rows x columns
__device__ __forceinline__ unsigned tap_mask(const ConvArgs& a, int hi0, int wi0) {
    unsigned vw = 0, mask = 0;
    // ks <= 3 (1 or 3 at the ABI; 2 for the stride-2 data gradient): three straight-line taps, no loop
#pragma unroll
    for (int kw = 0; kw < 3; ++kw) vw |= (unsigned)(kw < a.ks && wi0 + kw >= 0 && wi0 + kw < a.W) << kw;
#pragma unroll
    for (int kh = 0; kh < 3; ++kh)
        mask |= (kh < a.ks && hi0 + kh >= 0 && hi0 + kh < a.H) ? vw << (kh * a.ks) : 0u;
    return mask;
}
// element offset of the window's first pixel in the input tensor (64-bit; only dereferenced where the mask allows)
__device__ __forceinline__ long window_offset(const ConvArgs& a, int b, int hi0, int wi0) {
    return ((long)b * a.H * a.W + (long)hi0 * a.W + wi0) * a.in_cs;
}

// ---- epilogue math ------------------------------------------------------------------------------------------------------
// (pixel, channel) of an epilogue element in the tensors it addresses: the identity, or ConvArgs' depth-to-space map
__device__ __forceinline__ void epilogue_pos(const ConvArgs& a, int m, int n, long& pix, int& nn) {
    pix = m; nn = n;
    if (a.d2s_c) {
        int b, i, j;
        pixel_split(a, m, b, i, j);
        const int p = n / a.d2s_c;
        nn = n - p * a.d2s_c;
        pix = ((long)(b * 2 * a.Ho + 2 * i + (p >> 1))) * (2 * a.Wo) + 2 * j + (p & 1);
    }
}

__device__ __forceinline__ float silu(float x) {
    return x * __builtin_amdgcn_rcpf(1.0f + __builtin_amdgcn_exp2f(-1.44269504088896341f * x));
}
// The same formula on channel pairs: packed fp32 (v_pk_add/mul_f32 do two channels per issue slot; the two transcendentals
// stay per element) — the conv epilogues are VALU-bound on exactly this (128 SiLUs per lane in the 256x256 kernel).
__device__ __forceinline__ f32x2 silu_pk(f32x2 x) {
    const f32x2 u = x * -1.44269504088896341f;
    f32x2 e = {__builtin_amdgcn_exp2f(u.x), __builtin_amdgcn_exp2f(u.y)};
    e = e + 1.0f;
    const f32x2 r = {__builtin_amdgcn_rcpf(e.x), __builtin_amdgcn_rcpf(e.y)};
    return x * r;
}
// silu of a bf16 pair, rounded back to bf16 (the training forward's second output)
__device__ __forceinline__ unsigned silu_bf16x2(unsigned v) {
    const f32x2 y = silu_pk(f32x2{__uint_as_float(v << 16), __uint_as_float(v & 0xFFFF0000u)});
    return __builtin_bit_cast(unsigned, __builtin_convertvector(y, bf16x2));
}
// g * silu'(p) on a bf16 pair, rounded back to bf16 — THE formula of the backward (k_silu_bwd and the conv epilogues that
// absorb it must agree bit for bit, hence the explicit fma: nothing is left to contraction).
// silu'(p) = s + p s (1 - s), s = sigmoid(p)
__device__ __forceinline__ float dsilu_f32(float g, float p) {
    const float s = __builtin_amdgcn_rcpf(1.0f + __builtin_amdgcn_exp2f(-1.44269504088896341f * p));
    return g * __builtin_fmaf(p * s, 1.0f - s, s);
}
__device__ __forceinline__ unsigned dsilu_bf16x2(unsigned g, unsigned p) {
    const f32x2 y = {dsilu_f32(__uint_as_float(g << 16), __uint_as_float(p << 16)),
                     dsilu_f32(__uint_as_float(g & 0xFFFF0000u), __uint_as_float(p & 0xFFFF0000u))};
    return __builtin_bit_cast(unsigned, __builtin_convertvector(y, bf16x2));
}
// four consecutive channels: SiLU (compile-time), round to bf16 (v_cvt_pk_bf16_f32) -> two packed words
template <bool SILU>
__device__ __forceinline__ void act_pack4(f32x2 x0, f32x2 x1, unsigned& lo, unsigned& hi) {
    if (SILU) { x0 = silu_pk(x0); x1 = silu_pk(x1); }
    lo = __builtin_bit_cast(unsigned, __builtin_convertvector(x0, bf16x2));
    hi = __builtin_bit_cast(unsigned, __builtin_convertvector(x1, bf16x2));
}
// ... behind the bias add
template <bool SILU>
__device__ __forceinline__ void bias_act_pack4(float a0, float a1, float a2, float a3, const float4 b, unsigned& lo, unsigned& hi) {
    act_pack4<SILU>(f32x2{a0, a1} + f32x2{b.x, b.y}, f32x2{a2, a3} + f32x2{b.z, b.w}, lo, hi);
}

}  // namespace adayolo
