// What the LDS-DMA ring conv kernels (yolo_tile_pp.h, yolo_tile_pp128.h, yolo_conv_pq.hip) have in common, once: the k-tile
// position, the MFMA fragment addressing of both shapes, the accumulator helpers and the pieces of the wave-private transposing
// epilogue with its training contracts. Pieces, not a kernel: every k-loop, its ring and its wave grid stay in the kernel's own
// file, and so does what only one kernel does (the fused second layer, the chain's look-ahead and written-through stores, the
// measurement forms). Everything is __forceinline__ and takes compile-time tags: a kernel instantiates the forms it names.
// (The ladder from ConvArgs' act / res / pre / gpre / d2s_c onto those tags stays written out in each kernel: handed through a shared
// function the same ladder comes out of hipcc with another block order and wait list in yolo_tile_pp128.h and yolo_conv_pq.hip.)
#pragma once
#include "yolo_device.h"
#include <type_traits>

namespace adayolo {

// ---- k position ---------------------------------------------------------------------------------------------------------
// wave-uniform state of the k-tile a stage call addresses: channel chunk c0 of tap (kh, kw), byte offsets into a row's window /
// a weight row
struct KPos {
    int c0, kh, kw, tap;
    long aoff, woff;
};
__device__ __forceinline__ void kpos_offsets(const ConvArgs& a, KPos& p) {
    p.aoff = 2 * (((long)p.kh * a.W + p.kw) * a.in_cs + p.c0);
    p.woff = 2 * ((long)p.tap * a.Cin + p.c0);
}
// the next k-tile: channel chunks inner, taps outer
template <int BK>
__device__ __forceinline__ void kpos_advance(const ConvArgs& a, KPos& p) {
    p.c0 += BK;
    if (p.c0 >= a.Cin) {
        p.c0 = 0; ++p.tap; ++p.kw;
        if (p.kw == a.ks) { p.kw = 0; ++p.kh; }
    }
    kpos_offsets(a, p);
}
// k-tile t0 of a layer with cpt channel chunks per tap (where a split-K range starts)
template <int BK>
__device__ __forceinline__ KPos kpos_at(const ConvArgs& a, int t0, int cpt) {
    KPos p;
    p.tap = t0 / cpt; p.c0 = (t0 - p.tap * cpt) * BK;
    p.kh = p.tap / a.ks; p.kw = p.tap - p.kh * a.ks;
    kpos_offsets(a, p);
    return p;
}

// ---- fragments ----------------------------------------------------------------------------------------------------------
// A lane's place in an operand tile of 128-byte rows (BK = 64) whose 16-byte chunks are XOR-swizzled by (row >> 1) & 7.
// MS 32 (32x32x16): tile row (lane & 31), 16-byte k-chunk 2*kk + (lane >> 5) — the key is the same for every fragment of this
// lane because fragment origins are multiples of 32 rows. MS 16 (16x16x32): tile row (lane & 15), k-chunk 4*k2 + (lane >> 4),
// the same key rule — fragment origins are multiples of 16 rows; the 16 lanes of a row group read 16 distinct bank quads.
// koff[kk]: byte offset of the lane's chunk inside its row, MS 32: k-step kk; MS 16: k-step kk & 1 (entries 2, 3 repeat 0, 1)
template <int MS>
__device__ __forceinline__ void frag_pos(int lane, int& frow, int (&koff)[4]) {
    static_assert(MS == 32 || MS == 16, "MFMA shape: 32x32x16 or 16x16x32");
    frow = MS == 32 ? lane & 31 : lane & 15;
    const int fq = MS == 32 ? lane >> 5 : lane >> 4, key = (frow >> 1) & 7;
#pragma unroll
    for (int kk = 0; kk < 4; ++kk) koff[kk] = MS == 32 ? ((2 * kk + fq) ^ key) << 4 : ((4 * (kk & 1) + fq) ^ key) << 4;
}

// accumulators of either shape, f32x16 acc[channel frag][pixel frag] / f32x4 acc16[16-channel frag][16-pixel frag]: cleared
// (the keep-alive of the measurement builds that drop the epilogue stays in the kernels: its "v"-constraint asm, moved into a
// function template of its own, fails hipcc's host pass as soon as two kernels of a file instantiate it)
template <class V, int N0, int N1>
__device__ __forceinline__ void acc_zero(V (&acc)[N0][N1]) {
#pragma unroll
    for (int i = 0; i < N0; ++i)
#pragma unroll
        for (int j = 0; j < N1; ++j)
#pragma unroll
            for (int e = 0; e < (int)(sizeof(V) / 4); ++e) acc[i][j][e] = 0.0f;
}
// ---- epilogue -----------------------------------------------------------------------------------------------------------
// D[row = channel][col = pixel]: a lane holds pixel (lane & 31) and channels 8*qd + 4*(lane >> 5) + (0..3) of every 32x32
// fragment. Each wave transposes its own pixels x 64 ch through a PRIVATE LDS region (pitch kEpiPitch = 144 B: 16-byte aligned
// rows, 2-way write conflicts at most) — no workgroup barrier, a wave's stores leave as soon as its own fragment is converted —
// 32 pixels (a row group) at a time, and writes whole 128-byte row segments (8 lanes x 16 B): lane -> row (lane >> 3) + 8 it of
// the group, channels 8 (lane & 7) .. + 8.
// (Storing 8/16-byte pieces straight from the fragment layout was measured 2x slower: 32 rows x 32 B per instruction instead of
// 8 rows x 128 B.)
// MS 16: D is col = lane & 15 (pixel), row = 4 * (lane >> 4) + reg (channel): the four registers of a 16x16 fragment are one
// 8-byte write at pixel row 16 pb + (lane & 15), channel 16 cb + 4 * (lane >> 4) (16 rows x 4 column groups per instruction at
// pitch 144 B: conflict-free); the read side and everything behind it are the same.

// where a lane's fragment words go in the wave's region `my`
template <int MS>
__device__ __forceinline__ unsigned char* epi_wr(unsigned char* my, int lane) {
    return MS == 32 ? my + (lane & 31) * kEpiPitch + 8 * (lane >> 5) : my + (lane & 15) * kEpiPitch + 8 * (lane >> 4);
}
// the bias of the lane's channels; bias_w: the wave's 64 channels. MS 16 fills bq[0][cb] only
template <int MS>
__device__ __forceinline__ void epi_bias(const float* bias_w, int lane, float4 (&bq)[2][4]) {
#pragma unroll
    for (int ni = 0; ni < 2; ++ni)
#pragma unroll
        for (int qd = 0; qd < 4; ++qd)
            if (MS == 32) bq[ni][qd] = *reinterpret_cast<const float4*>(bias_w + ni * 32 + 8 * qd + 4 * (lane >> 5));
            else if (ni == 0) bq[0][qd] = *reinterpret_cast<const float4*>(bias_w + 16 * qd + 4 * (lane >> 4));
}
// row group mi: fragments + bias, activation (compile-time), bf16 -> the wave's region. MS 32 ...
template <bool SILU, int MI>
__device__ __forceinline__ void epi_put(const f32x16 (&acc)[2][MI], int mi, const float4 (&bq)[2][4], unsigned char* wr) {
#pragma unroll
    for (int ni = 0; ni < 2; ++ni)
#pragma unroll
        for (int qd = 0; qd < 4; ++qd) {
            unsigned lo, hi;
            bias_act_pack4<SILU>(acc[ni][mi][4 * qd], acc[ni][mi][4 * qd + 1], acc[ni][mi][4 * qd + 2], acc[ni][mi][4 * qd + 3],
                                 bq[ni][qd], lo, hi);
            *reinterpret_cast<u32x2*>(wr + mi * 32 * kEpiPitch + (ni * 32 + 8 * qd) * 2) = u32x2{lo, hi};
        }
}
// ... MS 32 with the bias already in the accumulators ...
template <bool SILU, int MI>
__device__ __forceinline__ void epi_put(const f32x16 (&acc)[2][MI], int mi, unsigned char* wr) {
#pragma unroll
    for (int ni = 0; ni < 2; ++ni)
#pragma unroll
        for (int qd = 0; qd < 4; ++qd) {
            unsigned lo, hi;
            act_pack4<SILU>(f32x2{acc[ni][mi][4 * qd], acc[ni][mi][4 * qd + 1]}, f32x2{acc[ni][mi][4 * qd + 2], acc[ni][mi][4 * qd + 3]}, lo, hi);
            *reinterpret_cast<u32x2*>(wr + mi * 32 * kEpiPitch + (ni * 32 + 8 * qd) * 2) = u32x2{lo, hi};
        }
}
// ... MS 16 (ni: the 16-pixel fragment of the group, qd: the 16-channel fragment)
template <bool SILU, int NP>
__device__ __forceinline__ void epi_put(const f32x4 (&acc16)[4][NP], int mi, const float4 (&bq)[2][4], unsigned char* wr) {
#pragma unroll
    for (int ni = 0; ni < 2; ++ni)
#pragma unroll
        for (int qd = 0; qd < 4; ++qd) {
            unsigned lo, hi;
            const f32x4 d = acc16[qd][2 * mi + ni];
            bias_act_pack4<SILU>(d[0], d[1], d[2], d[3], bq[0][qd], lo, hi);
            *reinterpret_cast<u32x2*>(wr + (2 * mi + ni) * 16 * kEpiPitch + 16 * qd * 2) = u32x2{lo, hi};
        }
}
// the four 16-byte row pieces of row group mi this lane stores; rd: the lane's piece of the group's first row
__device__ __forceinline__ void epi_rows(const unsigned char* rd, int mi, u32x4 (&v)[4]) {
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");  // same wave wrote and reads: in-order LDS, no barrier
#pragma unroll
    for (int it = 0; it < 4; ++it) v[it] = *reinterpret_cast<const u32x4*>(rd + (mi * 32 + it * 8) * kEpiPitch);
}
// v = bf16(v + r) on the packed pairs
__device__ __forceinline__ void epi_add_res(u32x4 (&v)[4], const u32x4 (&r)[4]) {
#pragma unroll
    for (int it = 0; it < 4; ++it)
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const f32x2 x = f32x2{__uint_as_float(v[it][j] << 16), __uint_as_float(v[it][j] & 0xFFFF0000u)} +
                            f32x2{__uint_as_float(r[it][j] << 16), __uint_as_float(r[it][j] & 0xFFFF0000u)};
            v[it][j] = pack_bf16x2(x.x, x.y);
        }
}
// element offset of row `it` of group mi (first row mrow, channel n) in a tensor of channel stride cs — or, D2S (stride-2 data
// gradient), of its depth-to-space image (px[it], nn): epilogue_pos
template <bool D2S>
__device__ __forceinline__ long epi_elem(int mrow, int n, int mi, int it, int cs, const long (&px)[4], int nn) {
    return D2S ? px[it] * cs + nn : (long)(mrow + 8 * (4 * mi + it)) * cs + n;
}
// THE training-forward contract (kKeep): the rows went through LDS as the bf16 PRE-activation; they are stored to a.pre and the
// activation (ACT) is applied to that ROUNDED value — bit for bit what adayolo_silu_fwd makes of it
template <bool ACT>
__device__ __forceinline__ void epi_keep(const ConvArgs& a, int mrow, int n, int mi, const bool (&ok)[4], u32x4 (&v)[4]) {
#pragma unroll
    for (int it = 0; it < 4; ++it) {
        if (ok[it]) *reinterpret_cast<u32x4*>(a.pre + (long)(mrow + 8 * (4 * mi + it)) * a.pre_cs + n) = v[it];
        if (ACT) {
#pragma unroll
            for (int j = 0; j < 4; ++j) v[it][j] = silu_bf16x2(v[it][j]);
        }
    }
}
// THE backward contract (kDs): v (the conv result + residual) is dL/d(layer output), stored to `out` (the lane's row pointers:
// op + row * ostep, or D2S) when a.out is set; a.gpre = bf16(v * silu'(a.pre)) — adayolo_silu_bwd inside the producing launch
template <bool D2S>
__device__ __forceinline__ void epi_ds(const ConvArgs& a, int mrow, int n, int mi, const bool (&ok)[4], unsigned short* op, long ostep,
                                       const long (&px)[4], int nn, u32x4 (&v)[4]) {
    // (four named rows, not a loop over an array: with `p[it] = 0; if (ok[it]) p[it] = load` in this inlined function hipcc keeps
    // the zero fill and the masked loads apart — +30 registers in yolo_conv_pq.hip's kernels against the same text in the kernel)
    u32x4 p0 = {0u, 0u, 0u, 0u}, p1 = p0, p2 = p0, p3 = p0;
    if (ok[0]) p0 = *reinterpret_cast<const u32x4*>(a.pre + epi_elem<D2S>(mrow, n, mi, 0, a.pre_cs, px, nn));
    if (ok[1]) p1 = *reinterpret_cast<const u32x4*>(a.pre + epi_elem<D2S>(mrow, n, mi, 1, a.pre_cs, px, nn));
    if (ok[2]) p2 = *reinterpret_cast<const u32x4*>(a.pre + epi_elem<D2S>(mrow, n, mi, 2, a.pre_cs, px, nn));
    if (ok[3]) p3 = *reinterpret_cast<const u32x4*>(a.pre + epi_elem<D2S>(mrow, n, mi, 3, a.pre_cs, px, nn));
    const u32x4 p[4] = {p0, p1, p2, p3};
    if (a.out) {
#pragma unroll
        for (int it = 0; it < 4; ++it)
            if (ok[it])
                __builtin_nontemporal_store(v[it], reinterpret_cast<u32x4*>(D2S ? a.out + px[it] * a.out_cs + nn : op + (4 * mi + it) * ostep));
    }
#pragma unroll
    for (int it = 0; it < 4; ++it) {
#pragma unroll
        for (int j = 0; j < 4; ++j) v[it][j] = dsilu_bf16x2(v[it][j], p[it][j]);
        if (ok[it]) __builtin_nontemporal_store(v[it], reinterpret_cast<u32x4*>(a.gpre + epi_elem<D2S>(mrow, n, mi, it, a.gpre_cs, px, nn)));
    }
}
// ... for a kernel without the depth-to-space form
__device__ __forceinline__ void epi_ds(const ConvArgs& a, int mrow, int n, int mi, const bool (&ok)[4], unsigned short* op, long ostep,
                                       u32x4 (&v)[4]) {
    const long px[4] = {0, 0, 0, 0};
    epi_ds<false>(a, mrow, n, mi, ok, op, ostep, px, n, v);
}

}  // namespace adayolo
