// Conv + bias + SiLU (+ residual) — implicit GEMM, 256 px x 128 ch tile, two wave groups in ping-pong, 3-deep ring.
//
// Sibling of yolo_tile_pp.h for the layers it cannot serve well: Cout = 128 (its tile is 256 channels wide) and
// small pixel counts where 256x256 tiles leave half the CUs idle (8x23x40 px: 116 tiles; here 232). Same ideas —
// waves 0-3 / 4-7 staggered by one barrier so that one wave of each SIMD issues MFMAs while the other reads
// fragments, LDS-DMA issued in the MFMA sections behind counted waits — with a different decomposition:
//
//   * wave grid 4 (px) x 2 (ch): wave tile 64 px x 64 ch (four 32x32 accumulators), the channel half is the
//     ping-pong group. Per k-tile (BK = 64) a wave reads 8 activation + 8 weight fragments for 16 MFMAs (a
//     2 x 4 grid with 128 x 32 wave tiles would need 20): LDS read + DMA write time stays below the MFMA time;
//   * a k-tile is TWO phases of 8 MFMAs (channel fragment 0, then 1). The activation fragments are read in P1's load
//     section, both weight fragments of the phase pair — W1 of this k-tile and W0 of the NEXT — in P2's: 8 reads per
//     load section; three weight register sets rotate;
//   * with two phases per k-tile a 2-buffer ring leaves one phase of DMA latency, so the ring is 3 k-tiles deep
//     (3 x 48 KB). Slots are units of what one load section reads: A (4 DMA instructions per wave), W0, W1 (1 each):
//         MFMA section of P1(t): issues W1(t+2), W0(t+3)  then s_waitcnt vmcnt(8)
//         MFMA section of P2(t): issues A(t+3)            then s_waitcnt vmcnt(10)
//     i.e. everything issued three phases ago is retired, and is first read two phases later (the distance the
//     stagger needs): issue -> read = 5 phases. A slot is re-staged at least one phase after its last read.
//
//   * MS (see yolo_tile_pp.h): 32 = v_mfma_f32_32x32x16_bf16 as above; 16 = v_mfma_f32_16x16x32_bf16 on the same wave
//     tile and schedule — 16 MFMAs per phase (four 16 px x two 16 ch fragments x two K = 32 steps), f32x4 acc[4][4], the DMA
//     pieces behind the 2nd, 6th, 10th and 14th MFMA. The split-K partials are stored in the shape's own lane order: writer
//     and reducer of a launch are the same instantiation.
//
// Restrictions (the launcher falls back otherwise): Cin % 64 == 0, Cout % 128 == 0.
// Measured and dropped (round 2, same outputs bit for bit): ONE phase per k-tile — all 16 fragments in one load section, 16
// MFMAs per section, two barriers per k-tile instead of four, 190 registers — 71 vs 70 us on 512 -> 1024 @ 8x23x40; the same
// with the six DMA pieces issued in the LOAD section so that the MFMA section is MFMAs only: 88 us (a piece costs the issuing
// wave ~150 cycles there, four waves at once). The barriers are not what holds this kernel; the operand stream is
// (profiles/round2_conv_pp_ablation.txt).
#pragma once
#include "yolo_ring.h"
#include "yolo_chain.h"
#ifndef PP_PRIO_MODE
#define PP_PRIO_MODE 0      // 0: s_setprio 1 around every MFMA section (default); 1: no priority; 2: static priority for the second wave group (measurement builds)
#endif

namespace adayolo {
namespace pp128 {

constexpr int BM = 256, BN = 128, BK = 64;
constexpr int kRow = BK * 2;                  // bytes per tile row
constexpr int kATile = BM * kRow;             // 32 KB
constexpr int kBuf = (BM + BN) * kRow;        // one k-tile: 48 KB
constexpr int kRing = 3 * kBuf;               // 144 KB
constexpr int kSmem = kRing + BN * 4 + 16;    // + bias + the split-K ticket; the epilogue (8 x 64 x 144 B = 72 KB) overlays the finished ring

// ABL: 0 real kernel, 5 no DMA instructions in the k-loop, 6 no epilogue, 7 activation DMA for one tap in nine
// (measurement builds; profiles/round2_conv_pp_ablation.txt)
//
// SPLIT (variants 100 + S, round 3): the k-tiles of one output tile are cut into S = a.ksplit equal ranges, one workgroup
// each — for the layers whose pixel count leaves most CUs without a tile (8 x 16 x 16 px at 1024 channels: 32 tiles of 144
// k-tiles; the training shapes of config 4). Every workgroup stores its fp32 accumulators to a.partial in its own lane
// order (16 B per lane, 1 KB per wave and instruction), takes a ticket of the tile, and the workgroup that draws the last
// one adds the S partial tiles IN SPLIT ORDER (its own included, read back: the sum does not depend on who arrives last)
// and runs the ordinary epilogue. The partials may cross XCDs, i.e. L2s: they are stored and loaded at device scope (sc1)
// and ordered by s_waitcnt vmcnt(0) + the ticket atomic — NOT by __threadfence(), whose release is a write-back of the
// whole L2 per workgroup (measured on 1024 -> 512 k3 @ 8x16x16, S = 8: k-loop 18.8 us, + partial stores 23.4, + fence and
// ticket 97; with sc1 accesses instead 27.8, + the last workgroup's S x 128 KB read-back and epilogue 43).
// Workgroup -> (tile, range) with the range varying fastest: the S workgroups of a tile are neighbours on one XCD
// (2-4 us better than tile-fastest).
// CHAIN (yolo_chain.h): the tile is a work item of the persistent chain kernel — `gid` is handed in, the outputs leave as
// written-through stores, the previous tile of the workgroup is published behind the prologue, wave 0 looks ahead.
template <int ABL, bool SPLIT, bool CHAIN, int MS = 32>
__device__ __forceinline__ void conv_tile(const ConvArgs& a, const int gid, unsigned char* smem, ChainCtx& cx) {
    static_assert(!(SPLIT && CHAIN), "the chain runs whole tiles");
    float* bias_s = reinterpret_cast<float*>(smem + kRing);
    int* ticket_s = reinterpret_cast<int*>(smem + kRing + BN * 4);

    int tid_ = threadIdx.x;
    if (CHAIN) asm volatile("" : "+v"(tid_));            // (nothing derived from the thread index is hoisted out of the chain's loop)
    const int tid = tid_, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int wm = wave & 3, wn = wave >> 2;             // wn is also the ping-pong group
    const int lid = SPLIT ? gid / a.ksplit : gid, kpart = SPLIT ? gid - lid * a.ksplit : 0;   // the ranges of a tile are neighbours
    ChainLook look;
    auto sched_stage = [&](int stage) {
        if (CHAIN && wave == 0) look.stage(stage, *cx.c, smem + kChainSchedOff, lane);
    };
    const int m0 = (lid / a.ntiles) * BM, n0 = (lid % a.ntiles) * BN;
    const unsigned long long zaddr = (unsigned long long)(const void*)g_zero16;

    // ---- per-row DMA state: one DMA instruction moves 8 tile rows. Activations: 32 instructions per k-tile, this
    //      wave issues the four of rows [32*wave, 32*wave + 32). Weights: unit W0 = rows [0,32) + [64,96) (channel
    //      fragment 0 of both groups), W1 = the other 64 rows; one instruction per wave and unit.
    const int slot = lane & 7, rsub = lane >> 3;
    unsigned long long arow[4], wrow[2];
    unsigned amask[4];
#pragma unroll
    for (int u = 0; u < 2; ++u) {
        const int r = (wave >> 2) * 64 + u * 32 + (wave & 3) * 8 + rsub;
        const int q = slot ^ ((r >> 1) & 7);
        wrow[u] = (unsigned long long)(a.w + (long)(n0 + r) * (a.ks * a.ks * a.Cin) + 8 * q);
    }
    const int wlds0 = kATile + ((wave >> 2) * 64 + (wave & 3) * 8) * kRow;       // unit W0; W1 = + 32 rows
    const int alds0 = wave * 32 * kRow;                                          // + 8 rows per instruction
    auto decode_rows = [&]() {
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int r = wave * 32 + i * 8 + rsub;
            const int q = slot ^ ((r >> 1) & 7);
            const int m = m0 + r;
            unsigned mask = 0;
            long off = 0;
            if (m < a.M) {
                int b, hi0, wi0;
                window_origin(a, m, b, hi0, wi0);
                mask = tap_mask(a, hi0, wi0);
                off = window_offset(a, b, hi0, wi0) + 8 * q;
            }
            amask[i] = mask;
            arow[i] = (unsigned long long)(a.in + off);
        }
    };
    const int cpt = a.Cin / BK;
    const int nK = SPLIT ? a.ks * a.ks * cpt / a.ksplit : a.ks * a.ks * cpt;     // k-tiles of THIS workgroup

    auto advance = [&](KPos& p) { kpos_advance<BK>(a, p); };
    auto stage_a1 = [&](int i, unsigned char* buf, const KPos& p, bool live) {
        if (ABL == 5 && !live) return;
        const bool ok = live && ((amask[i] >> p.tap) & 1u);
        dma16(sel(ok, arow[i] + p.aoff, zaddr), buf + alds0 + i * 8 * kRow);
    };
    auto stage_w1 = [&](int u, unsigned char* buf, const KPos& p, bool live) {
        if (ABL == 5 && !live) return;
        dma16(sel(live, wrow[u] + p.woff, zaddr), buf + wlds0 + u * 32 * kRow);
    };
    auto stage_a = [&](unsigned char* buf, const KPos& p, bool live) {
#pragma unroll
        for (int i = 0; i < 4; ++i) stage_a1(i, buf, p, live);
    };

    // ---- prologue, in the steady-state issue order: W0(0); A(0); W1(0), W0(1); A(1); W1(1), W0(2); A(2)
    KPos q0{0, 0, 0, 0, 0, 0};
    if (SPLIT) q0 = kpos_at<BK>(a, kpart * nK, cpt);     // first k-tile of this workgroup's range
    KPos q1 = q0; advance(q1);
    KPos q2 = q1; advance(q2);
    if (wave == 0 && lane < 32) dma16((unsigned long long)(a.bias + n0) + 16 * lane, bias_s);   // 512 B: half a wave
    stage_w1(0, smem, q0, true);
    decode_rows();
    stage_a(smem, q0, true);
    stage_w1(1, smem, q0, true);
    stage_w1(0, smem + kBuf, q1, 1 < nK);
    stage_a(smem + kBuf, q1, 1 < nK);
    stage_w1(1, smem + kBuf, q1, 1 < nK);
    stage_w1(0, smem + 2 * kBuf, q2, 2 < nK);
    stage_a(smem + 2 * kBuf, q2, 2 < nK);
    if (CHAIN) {
        wait_vm<0>();                                    // ... and the previous tile's written-through stores are complete
        barrier();
        chain_publish(cx, tid);
        sched_stage(0);
    } else {
        wait_vm<10>();                                   // W0(0), A(0), W1(0), W0(1) landed (this wave's share)
        barrier();
    }

    f32x16 acc[2][2];                                    // [channel frag][pixel frag]
    f32x4 acc16[4][4];                                   // MS 16: [16-channel frag][16-pixel frag]; the same 64 registers
    if constexpr (MS == 32) acc_zero(acc);
    else acc_zero(acc16);

    // fragment addressing: frag_pos of yolo_ring.h, written out — through the shared function the split-K kernels, which sit at
    // 256 registers, come out with other spill counts (8 -> 4) and another wait list
    const int frow = MS == 32 ? lane & 31 : lane & 15, fq = MS == 32 ? lane >> 5 : lane >> 4, key = (frow >> 1) & 7;
    const int abase = (wm * 64 + frow) * kRow, wbase = kATile + (wn * 64 + frow) * kRow;
    int koff[4];
#pragma unroll
    for (int kk = 0; kk < 4; ++kk) koff[kk] = MS == 32 ? ((2 * kk + fq) ^ key) << 4 : ((4 * (kk & 1) + fq) ^ key) << 4;

    // MS 16: af[pf >> 1][2 * (pf & 1) + k2] is the 16-pixel fragment pf at k-step k2, w[2 * cf + k2] the 16-channel fragment cf
    // of the phase's half — the same 8 + 4 (+ 4) reads of the same rows
    bf16x8 af[2][4], wx[4], wy[4], wz[4];
    auto read_a = [&](const unsigned char* buf) {
#pragma unroll
        for (int mi = 0; mi < 2; ++mi)
#pragma unroll
            for (int kk = 0; kk < 4; ++kk)
                af[mi][kk] = MS == 32 ? *reinterpret_cast<const bf16x8*>(buf + abase + mi * 32 * kRow + koff[kk])
                                      : *reinterpret_cast<const bf16x8*>(buf + abase + (2 * mi + (kk >> 1)) * 16 * kRow + koff[kk]);
    };
    auto read_w = [&](const unsigned char* buf, int ni, bf16x8 (&w)[4]) {
#pragma unroll
        for (int kk = 0; kk < 4; ++kk)
            w[kk] = MS == 32 ? *reinterpret_cast<const bf16x8*>(buf + wbase + ni * 32 * kRow + koff[kk])
                             : *reinterpret_cast<const bf16x8*>(buf + wbase + (2 * ni + (kk >> 1)) * 16 * kRow + koff[kk]);
    };
    // MFMA section: 8 MFMAs, the phase's DMA instructions issued behind the 1st, 3rd, 5th and 7th, then the counted wait
    // source addresses are computed in the load section in front (see yolo_tile_pp.h): between two MFMAs only
    // s_mov m0 + the DMA instruction remain
    auto mma = [&](int ni, const bf16x8 (&w)[4], const unsigned long long (&g)[4], unsigned char* const (&d)[4], int npieces) {
#if PP_PRIO_MODE == 0
        __builtin_amdgcn_s_setprio(1);
#endif
        if constexpr (MS == 32) {
#pragma unroll
        for (int kk = 0; kk < 4; ++kk)
#pragma unroll
            for (int mi = 0; mi < 2; ++mi) {
                acc[ni][mi] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(w[kk], af[mi][kk], acc[ni][mi], 0, 0, 0);
                const int n = 2 * kk + mi;
                if ((n & 1) == 0 && (n >> 1) < npieces) {
                    __builtin_amdgcn_sched_barrier(0);
                    if (ABL != 5) dma16(g[n >> 1], d[n >> 1]);
                    __builtin_amdgcn_sched_barrier(0);
                }
            }
        } else {
            // k-step outer: every accumulator takes its two steps in ascending order, eight MFMAs apart; the DMA pieces at the
            // same points of the section (behind the 2nd, 6th, 10th and 14th MFMA of 16)
#pragma unroll
            for (int k2 = 0; k2 < 2; ++k2)
#pragma unroll
                for (int cf = 0; cf < 2; ++cf)
#pragma unroll
                    for (int pf = 0; pf < 4; ++pf) {
                        acc16[2 * ni + cf][pf] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(w[2 * cf + k2], af[pf >> 1][2 * (pf & 1) + k2],
                                                                                       acc16[2 * ni + cf][pf], 0, 0, 0);
                        const int n = 8 * k2 + 4 * cf + pf;
                        if ((n & 3) == 1 && (n >> 2) < npieces) {
                            __builtin_amdgcn_sched_barrier(0);
                            if (ABL != 5) dma16(g[n >> 2], d[n >> 2]);
                            __builtin_amdgcn_sched_barrier(0);
                        }
                    }
        }
#if PP_PRIO_MODE == 0
        __builtin_amdgcn_s_setprio(0);
#endif
    };

    read_w(smem, 0, wx);                                 // W0 of k-tile 0
#if PP_PRIO_MODE == 2
    if (wn == 1) __builtin_amdgcn_s_setprio(1);
#endif
    if (wn == 1) barrier();                              // stagger group 1 by one barrier

    KPos p2 = q2, p3 = q2;                               // p2: k-tile t+2, p3: k-tile t+3 (advanced inside the loop)
    // one k-tile: `b0` its buffer, `b1` / `b2` the buffers of k-tiles t+1 / t+2 (t+3 lands in b0 again)
    auto ktile = [&](unsigned char* b0, unsigned char* b1, unsigned char* b2, int t, bf16x8 (&w0)[4], bf16x8 (&w1)[4],
                     bf16x8 (&wnx)[4]) {
        const bool live2 = ABL != 5 && t + 2 < nK, live3 = ABL != 5 && t + 3 < nK;
        advance(p3);                                      // -> k-tile t+3
        // P1: channel fragment 0; stages W1(t+2), W0(t+3)
        read_a(b0);
        {
            unsigned long long g[4] = {sel(live2, wrow[1] + p2.woff, zaddr), sel(live3, wrow[0] + p3.woff, zaddr), 0, 0};
            unsigned char* const d[4] = {b2 + wlds0 + 32 * kRow, b0 + wlds0, nullptr, nullptr};
            asm volatile("" : "+v"(g[0]), "+v"(g[1]));
            barrier();
            mma(0, w0, g, d, 2);
        }
        wait_vm<8>();
        barrier();
        // P2: channel fragment 1; the load section also fetches W0 of the NEXT k-tile; stages A(t+3)
        read_w(b0, 1, w1);
        read_w(b1, 0, wnx);
        {
            unsigned long long g[4];
            unsigned char* d[4];
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                g[j] = sel(live3 && ((amask[j] >> p3.tap) & 1u), arow[j] + p3.aoff, zaddr);
                d[j] = b0 + alds0 + j * 8 * kRow;
            }
            asm volatile("" : "+v"(g[0]), "+v"(g[1]), "+v"(g[2]), "+v"(g[3]));
            barrier();
            unsigned char* const dc[4] = {d[0], d[1], d[2], d[3]};
            mma(1, w1, g, dc, (ABL == 7 && p3.tap != 0) ? 0 : 4);   // ABL 7 (measurement): activation DMA for one tap in nine
        }
        wait_vm<10>();
        barrier();
        p2 = p3;
    };
    unsigned char* B0 = smem;
    unsigned char* B1 = smem + kBuf;
    unsigned char* B2 = smem + 2 * kBuf;
    for (int t = 0; t < nK; t += 3) {
        ktile(B0, B1, B2, t, wx, wy, wz);
        if (t + 1 < nK) ktile(B1, B2, B0, t + 1, wz, wx, wy);
        if (t + 2 < nK) ktile(B2, B0, B1, t + 2, wy, wz, wx);
    }
    asm volatile("" ::"v"(wx[0]), "v"(wy[0]), "v"(wz[0]));
    if (wn == 0) barrier();                              // pairs with group 1's last barrier
    wait_vm<0>();                                        // the tail's zero-fill DMAs target the ring the epilogue overlays
    barrier();
    if (ABL == 6) {
        if constexpr (MS == 32) {
#pragma unroll
        for (int ni = 0; ni < 2; ++ni)
#pragma unroll
            for (int mi = 0; mi < 2; ++mi) asm volatile("" ::"v"(acc[ni][mi]));
        } else {
#pragma unroll
            for (int cf = 0; cf < 4; ++cf)
#pragma unroll
                for (int pf = 0; pf < 4; ++pf) asm volatile("" ::"v"(acc16[cf][pf]));
        }
        return;
    }

    if constexpr (SPLIT) {
        // partial tiles cross XCDs, i.e. L2s: stores and loads at DEVICE scope (sc1: written through / read past the
        // non-coherent lines), ordered by s_waitcnt + the ticket — a __threadfence() here is a whole-L2 write-back per
        // workgroup (measured: +70 us on a 25 us launch)
        constexpr int kSc1 = 16;
        const int S = a.ksplit;
        const __amdgpu_buffer_rsrc_t rsP = __builtin_amdgcn_make_buffer_rsrc(
            (void*)(a.partial + (long)lid * S * (BM * BN)), 0, 0xFFFFFF00u, 0x00020000u);
        const int mine = (kpart * 16 * 512 + tid) * 16;              // byte offset of this lane's first 16 B
#pragma unroll
        for (int ni = 0; ni < 2; ++ni)
#pragma unroll
            for (int mi = 0; mi < 2; ++mi)
#pragma unroll
                for (int g = 0; g < 4; ++g) {
                    // (MS 16: the sixteen f32x4 accumulators in their own order — ni * 2 + mi the channel, g the pixel fragment)
                    const u32x4 v = MS == 32 ? u32x4{__float_as_uint(acc[ni][mi][4 * g]), __float_as_uint(acc[ni][mi][4 * g + 1]),
                                                     __float_as_uint(acc[ni][mi][4 * g + 2]), __float_as_uint(acc[ni][mi][4 * g + 3])}
                                             : __builtin_bit_cast(u32x4, acc16[ni * 2 + mi][g]);
                    __builtin_amdgcn_raw_buffer_store_b128(v, rsP, mine + ((ni * 2 + mi) * 4 + g) * (512 * 16), 0, kSc1);
                }
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");   // this wave's partials are written through
        __syncthreads();
        if (tid == 0) *ticket_s = __hip_atomic_fetch_add(a.tickets + lid, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        __syncthreads();
        if (*ticket_s != S - 1) return;
        if (tid == 0) __hip_atomic_store(a.tickets + lid, 0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);   // for the next launch
#pragma unroll
        for (int ni = 0; ni < 2; ++ni)
#pragma unroll
            for (int mi = 0; mi < 2; ++mi)
#pragma unroll
                for (int e = 0; e < 16; ++e) {
                    if (MS == 32) acc[ni][mi][e] = 0.0f;
                    else acc16[ni * 2 + mi][e >> 2][e & 3] = 0.0f;
                }
        // S rounds of 16 loads per lane, the next round in flight while this one is added (a reducing CU pulls S x 128 KB)
        u32x4 va[16], vb[16];
        auto fetch = [&](u32x4 (&v)[16], int sp) {
            const int src = (sp * 16 * 512 + tid) * 16;
#pragma unroll
            for (int j = 0; j < 16; ++j)
                v[j] = __builtin_bit_cast(u32x4, __builtin_amdgcn_raw_buffer_load_b128(rsP, src + j * (512 * 16), 0, kSc1));
        };
        auto add = [&](const u32x4 (&v)[16]) {
#pragma unroll
            for (int ni = 0; ni < 2; ++ni)
#pragma unroll
                for (int mi = 0; mi < 2; ++mi)
#pragma unroll
                    for (int g = 0; g < 4; ++g)
#pragma unroll
                        for (int c = 0; c < 4; ++c) {
                            if (MS == 32) acc[ni][mi][4 * g + c] += __uint_as_float(v[(ni * 2 + mi) * 4 + g][c]);
                            else acc16[ni * 2 + mi][g][c] += __uint_as_float(v[(ni * 2 + mi) * 4 + g][c]);
                        }
        };
        fetch(va, 0);
        for (int sp = 0; sp < S; sp += 2) {
            if (sp + 1 < S) fetch(vb, sp + 1);
            add(va);
            if (sp + 2 < S) fetch(va, sp + 2);
            if (sp + 1 < S) add(vb);
        }
    }

    // ---- epilogue: wave-private LDS transpose (the pieces: yolo_ring.h), 32 px x 64 ch at a time, 128-byte row segments
    unsigned char* my = smem + wave * (64 * kEpiPitch);
    __amdgpu_buffer_rsrc_t rs_out;                       // CHAIN: written-through (sc1) stores, 32-bit byte offsets
    if (CHAIN) rs_out = __builtin_amdgcn_make_buffer_rsrc((void*)a.out, 0, 0x7FFFFFFF, 0x00020000);
    // see yolo_tile_pp.h: compile-time activation / residual copies, bias and pointers hoisted, batched reads and stores
    auto epilogue = [&](auto silu_tag, auto res_tag, auto keep_tag, auto ds_tag, auto d2s_tag) {
        // kKeep: the tile goes through LDS as the bf16 PRE-activation (kSilu off), then epi_keep
        // kDs (backward): epi_ds
        // kD2s (stride-2 data gradient): every tensor the epilogue touches is addressed depth-to-space (epilogue_pos)
        constexpr bool kKeep = decltype(keep_tag)::value, kAct = decltype(silu_tag)::value, kDs = decltype(ds_tag)::value;
        constexpr bool kSilu = kAct && !kKeep, kRes = decltype(res_tag)::value, kD2s = decltype(d2s_tag)::value;
        static_assert(!(kD2s && (kKeep || kAct)), "depth-to-space addressing serves the backward forms only");
        float4 bq[2][4];
        epi_bias<MS>(bias_s + wn * 64, lane, bq);
        const int chunk = lane & 7, r0 = lane >> 3;
        const int mrow = m0 + wm * 64 + r0, n = n0 + wn * 64 + chunk * 8;
        unsigned short* const op = a.out + (long)mrow * a.out_cs + n;
        const unsigned short* const rp = kRes ? a.res + (long)mrow * a.res_cs + n : nullptr;
        const long ostep = 8L * a.out_cs, rstep = kRes ? 8L * a.res_cs : 0;
        unsigned char* const wr = epi_wr<MS>(my, lane);
        const unsigned char* const rd = my + r0 * kEpiPitch + chunk * 16;
        const int obyte = CHAIN ? (int)(((long)mrow * a.out_cs + n) * 2) : 0;
#pragma unroll
        for (int mi = 0; mi < 2; ++mi) {
            sched_stage(mi + 1);                                 // CHAIN look-ahead: records, then arrival counters
            u32x4 v[4], r[4];
            bool ok[4];
#pragma unroll
            for (int it = 0; it < 4; ++it) ok[it] = mrow + 8 * (4 * mi + it) < a.M;
            long px[4];                                          // kD2s: the pixel each row lands on, nn its channel there
            int nn = n;
            if (kD2s) {
#pragma unroll
                for (int it = 0; it < 4; ++it) epilogue_pos(a, ok[it] ? mrow + 8 * (4 * mi + it) : 0, n, px[it], nn);
            }
            if (kRes) {                                          // in flight while this group's SiLUs are computed
#pragma unroll
                for (int it = 0; it < 4; ++it) {
                    r[it] = u32x4{0u, 0u, 0u, 0u};
                    if (ok[it]) r[it] = *reinterpret_cast<const u32x4*>(kD2s ? a.res + px[it] * a.res_cs + nn : rp + (4 * mi + it) * rstep);
                }
            }
            if constexpr (MS == 32) epi_put<kSilu>(acc, mi, bq, wr);
            else epi_put<kSilu>(acc16, mi, bq, wr);
            epi_rows(rd, mi, v);
            if (kKeep) epi_keep<kAct>(a, mrow, n, mi, ok, v);
            if (kRes) epi_add_res(v, r);
            if (kDs) {
                epi_ds<kD2s>(a, mrow, n, mi, ok, op, ostep, px, nn, v);
                continue;
            }
#pragma unroll
            for (int it = 0; it < 4; ++it)
                if (ok[it]) {
                    if (CHAIN) __builtin_amdgcn_raw_buffer_store_b128(v[it], rs_out, obyte + (4 * mi + it) * (int)(2 * ostep), 0, 16);
                    else __builtin_nontemporal_store(v[it], reinterpret_cast<u32x4*>(kD2s ? a.out + px[it] * a.out_cs + nn
                                                                                          : op + (4 * mi + it) * ostep));
                }
        }
    };
    const std::false_type no{};
    const std::true_type yes{};
    if constexpr (CHAIN) {                               // the chain runs the plain forward forms only (yolo_api.hip checks)
        if (a.act == ADAYOLO_ACT_SILU) { if (a.res) epilogue(yes, yes, no, no, no); else epilogue(yes, no, no, no, no); }
        else { if (a.res) epilogue(no, yes, no, no, no); else epilogue(no, no, no, no, no); }
    } else if (a.d2s_c) {                                // stride-2 data gradient (act none, no kept pre-activation)
        if (a.gpre) { if (a.res) epilogue(no, yes, no, yes, yes); else epilogue(no, no, no, yes, yes); }
        else { if (a.res) epilogue(no, yes, no, no, yes); else epilogue(no, no, no, no, yes); }
    } else if (a.gpre) {
        if (a.res) epilogue(no, yes, no, yes, no); else epilogue(no, no, no, yes, no);
    } else if (a.pre) {
        if (a.act == ADAYOLO_ACT_SILU) { if (a.res) epilogue(yes, yes, yes, no, no); else epilogue(yes, no, yes, no, no); }
        else { if (a.res) epilogue(no, yes, yes, no, no); else epilogue(no, no, yes, no, no); }
    } else if (a.act == ADAYOLO_ACT_SILU) {
        if (a.res) epilogue(yes, yes, no, no, no); else epilogue(yes, no, no, no, no);
    } else {
        if (a.res) epilogue(no, yes, no, no, no); else epilogue(no, no, no, no, no);
    }
    if (CHAIN) {
        sched_stage(3);
        barrier();                                       // the tile's LDS is free; {next item, ready, ...} is in place
    }
}

}  // namespace pp128
}  // namespace adayolo
