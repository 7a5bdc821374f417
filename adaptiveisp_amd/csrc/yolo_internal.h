// Host / launcher interface shared between the translation units of libadayolo.so (what the kernels share on the device
// side — vector types, helpers, epilogue math — is yolo_device.h).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "../../include/adayolo.h"

namespace adayolo {

// Host code starts from `ConvArgs{}` — every member zero or its default — and sets what the entry point uses (yolo_api.hip), so
// that a new field cannot be left uninitialised in one of them. (No default initialisers on the members below: the chain
// kernel declares a ConvArgs it fills from its tables.)
struct ConvArgs {
    const unsigned short* in; int in_cs;
    const unsigned short* w; const float* bias;
    const unsigned short* res; int res_cs;
    unsigned short* out; int out_cs;
    int B, H, W, Cin, Cout, Ho, Wo, ks, stride, pad, act;
    int M;            // B*Ho*Wo
    int mtiles, ntiles;
    // division by Ho*Wo and by Wo as multiply-high + shift (exact for 0 <= n < 2^31; sh < 0: divisor is 1)
    unsigned magic_hw, magic_w;
    int sh_hw, sh_w;
    // fused second layer (yolo_tile_pp.h, Cout == 256 only): a 1x1 conv 256 -> 128 + bias + SiLU applied to this conv's
    // OUTPUT tile while it is in LDS (Bottleneck.cv1 of the next block); null = not fused
    const unsigned short* w2; const float* bias2;
    unsigned short* out2; int out2_cs;
    // training forward (yolo_conv_dma2.hip / epi_keep of yolo_ring.h): when set, the bf16 pre-activation (conv + bias) is stored
    // here and the activation is applied to that ROUNDED value — bit for bit what adayolo_silu_fwd makes of it
    unsigned short* pre; int pre_cs;
    // split-K (yolo_tile_pp128.h, variants 100 + S): S workgroups per output tile, fp32 partial tiles + one ticket per tile
    // in the caller's workspace; 1 = every other kernel
    float* partial = nullptr; int* tickets = nullptr; int ksplit = 1;
    // backward of the frozen detector (variants of the keep set): when gpre is set, `pre` is an INPUT (the layer's saved
    // pre-activation), the conv result (+ residual) is the gradient of that layer's output — stored to `out` only when `out`
    // is not null — and gpre = bf16(that bf16 value * silu'(pre)): adayolo_silu_bwd inside the producing launch
    unsigned short* gpre = nullptr; int gpre_cs = 0;
    // data gradient of a stride-2 conv as a 2x2 stride-1 conv over the (small) output-gradient grid whose 4*C output channels
    // are the four pixel parities of the (large) input-gradient tensor: d2s_c = C > 0 makes the epilogue address out / res /
    // pre / gpre depth-to-space — channel group p of pixel (b, i, j) is pixel (b, 2i + p/2, 2j + p%2) of [B, 2Ho, 2Wo, C]
    int d2s_c = 0;
    // persistent chain (yolo_conv_chain.hip): which tile body runs this layer's items — 0: 256 x 256 (yolo_tile_pp.h),
    // 1: 256 x 128 (yolo_tile_pp128.h)
    int chain_tile = 0;
};

// One launch of a kernel whose dynamic LDS exceeds the 64 KB default. The attribute that allows it is set once per kernel — one
// instantiation of this template, hence one counter, per Kern (idempotent, benign if raced) — and again only if a launch asks
// for more than any before it (the measurement builds' *_EXTRA_SMEM switches).
template <auto Kern, class... Args>
hipError_t launch_lds(dim3 grid, dim3 block, int smem, hipStream_t s, const Args&... args) {
    static int allowed = 0;
    if (smem > allowed) {
        hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(Kern), hipFuncAttributeMaxDynamicSharedMemorySize, smem);
        if (e != hipSuccess) return e;
        allowed = smem;
    }
    hipLaunchKernelGGL(Kern, grid, block, smem, s, args...);
    return hipGetLastError();
}

// ---- persistent chain (yolo_conv_chain.hip: k_conv_chain): consecutive layers' tiles (256 x 256, 256 x 128) in ONE launch.
// One work item = one tile of one layer; the tables are built on the host (yolo_api.hip: adayolo_conv_chain_prepare).
// Workspace (device, caller-owned; the byte offsets are multiples of 64):
//   [0, 64)            int head (next item to hand out), int err (!= 0: a bounded wait of THIS launch gave up: item + 1), int exit
//                      (workgroups that have left), int sticky err (the last launch that gave up, until the next prepare),
//                      padding — head, err, exit and done[] are ZERO between launches
//   [64, ...)          int done[ndone]: arrival counters, one per (layer, m-tile)
//   [off_layers, ...)  ConvArgs[nlayers]
//   [off_heads, ...)   ChainHead[total]   layer-major: an item only ever waits for items BEFORE it in this order
//   [off_deps, ...)    ChainDeps[total]
// Everything behind the counters is constant during a launch and read through the SCALAR path (uniform indices).
struct ChainHead { int layer, lid, flag, pad; };   // tile `lid` (m-tile * ntiles + n-tile) of `layer`; done[flag] += 1 when it is stored
struct ChainDeps {                                 // done[lo .. lo + n) each >= need before the input window / the residual rows are read
    int in_lo, in_n_need;                          // (n << 16) | need; n = 0: produced before the launch
    int res_lo, res_n_need;
};
struct ChainArgs {
    unsigned char* ws;
    int* host_err;               // pinned HOST word (device-visible): the launch's last workgroup mirrors a give-up code there, so
                                 // that adayolo_conv_chain_poll reads it without touching the device (nullptr: not mirrored)
    int off_layers, off_heads, off_deps, total, ndone;
    int stagger;                 // cycles: workgroup b starts ((b >> 3) & 7) * stagger late (0: all at once). ADAYOLO_CHAIN_STAGGER
};
hipError_t launch_conv_chain(const ChainArgs& c, int grid, hipStream_t s);
// The MFMA shape the k-loop of a ring-kernel family runs on: 32 (v_mfma_f32_32x32x16_bf16) or 16 (v_mfma_f32_16x16x32_bf16).
// Process-wide, read by the launchers on the host at enqueue time (adayolo_set_mfma_shape / ADAYOLO_MFMA_SHAPE_PP, _PP128);
// the chain kernel runs each tile type on its family's shape.
enum ShapeFamily { kShapePp = 0, kShapePp128 = 1 };
int mfma_shape(ShapeFamily f);
hipError_t launch_conv_dma(ConvArgs a, hipStream_t s, int variant);   // LDS-DMA ring (yolo_conv_dma.hip)
hipError_t launch_conv_dma2(ConvArgs a, hipStream_t s, int variant);  // lean-address 32x32 MFMA ring (yolo_conv_dma2.hip)
hipError_t launch_conv_small(ConvArgs a, hipStream_t s, int variant); // 3x3, Cin 32/64, whole K resident (yolo_conv_small.hip)
hipError_t launch_conv_pp(ConvArgs a, hipStream_t s, int variant);    // 256x256 ping-pong wave groups (yolo_conv_pp.hip)
hipError_t launch_conv_pp128(ConvArgs a, hipStream_t s, int variant); // 256x128 ping-pong, 3-deep ring (yolo_conv_pp128.hip)
size_t conv_pp128_splitk_bytes(const ConvArgs& a, int S);               // workspace of the split-K form, 0 = shape not served
hipError_t launch_conv_pp128_splitk(ConvArgs a, hipStream_t s, int S, void* workspace, size_t workspace_bytes);
// one Bottleneck (1x1 256 -> 128 + SiLU, 3x3 128 -> 256 + SiLU, + x) per launch, hidden tensor in LDS (yolo_bneck.hip)
hipError_t launch_bottleneck256(const void* x, int x_cs, const void* w1, const float* b1, const void* w2, const float* b2,
                                void* out, int out_cs, int B, int H, int W, hipStream_t s);
// one Bottleneck of the shallow stages (C = 64 / 128) per launch: weights in registers, x patch by LDS-DMA, h in LDS (yolo_bneck_ws.hip)
hipError_t launch_bottleneck_ws(const void* x, int x_cs, const void* w1, const float* b1, const void* w2, const float* b2,
                                void* out, int out_cs, int B, int H, int W, int C, hipStream_t s);
hipError_t launch_conv_k1(ConvArgs a, hipStream_t s);                 // 1x1, whole K at once: weights in registers (fragment-major copy), activation tile in LDS (yolo_conv_k1.hip)
hipError_t launch_conv_pq(ConvArgs a, hipStream_t s, int variant);    // 256x128, 4 waves, two workgroups per CU (yolo_conv_pq.hip)
hipError_t launch_conv_ws(ConvArgs a, hipStream_t s, int variant);    // 3x3 s1, Cin 32 / 64: weights in registers, patch in LDS, persistent (yolo_conv_ws.hip)
hipError_t launch_stem(const float* img, const float* w, const float* bias, void* out, int out_cs, int B, int H,
                       int W, int Hp, int pad_top, float pad_value, int act, hipStream_t s, void* pre = nullptr, int pre_cs = 0);
hipError_t launch_letterbox_pack(const float* img, void* out, int out_cs, int B, int H, int W, int Hp, int pad_top,
                                 float pad_value, hipStream_t s);
hipError_t launch_stem_down(const float* img, const float* w0, const float* b0, const void* w1, const float* b1, void* out,
                            int out_cs, int B, int H, int W, int Hp, int pad_top, float pad_value, const void* w2,
                            const float* b2, void* out2, int out2_cs, hipStream_t s);
hipError_t launch_upsample2x(const void* in, int in_cs, void* out, int out_cs, int B, int H, int W, int C,
                             hipStream_t s);
hipError_t launch_detect_decode(const void* raw, int raw_cs, float* pred, int pred_rows, int row_offset,
                                const float* anchors_px, float det_stride, int B, int ny, int nx, int na, int no,
                                hipStream_t s);
hipError_t launch_silu_fwd(const void* pre, int pre_cs, const void* res, int res_cs, void* out, int out_cs, long npix,
                           int C, hipStream_t s);
hipError_t launch_silu_bwd(const void* gy, int gy_cs, const void* pre, int pre_cs, void* gp, int gp_cs, void* gres,
                           int gres_cs, int accumulate, long npix, int C, hipStream_t s);
hipError_t launch_zero_insert(const void* in, int in_cs, void* out, int out_cs, int B, int Ho, int Wo, int H, int W, int C,
                              hipStream_t s);
hipError_t launch_upsample_bwd(const void* gy, int gy_cs, void* gx, int gx_cs, int accumulate, int B, int H, int W, int C,
                               hipStream_t s);
// SPP's three max pools (5, 9, 13; stride 1) in one launch and their gradient in one (yolo_spp.hip)
hipError_t launch_spp_fwd(const void* x, int x_cs, void* out, int out_cs, int B, int H, int W, int C, hipStream_t s);
hipError_t launch_spp_bwd(const void* x, int x_cs, const void* gout, int go_cs, void* gx, int gx_cs, int accumulate, int B, int H,
                          int W, int C, hipStream_t s);
hipError_t launch_image_grad(const void* g, int g_cs, float* grad_img, int B, int H, int W, int Hp, int pad_top,
                             hipStream_t s);
hipError_t launch_detloss_fwd(const adayolo_loss_args& a, hipStream_t s);   // yolo_loss.hip
hipError_t launch_detloss_bwd(const adayolo_loss_args& a, hipStream_t s);
hipError_t launch_nms(const float* boxes, int n, float thr, int max_det, unsigned long long* mask_ws, int* keep,
                      int* num_keep, hipStream_t s);
hipError_t launch_match(const adayolo_match_args& a, hipStream_t s);          // yolo_match.hip
// whole-batch NMS (yolo_nms_batch.hip): the workspace's layout is a function of (B, cap, max_det) alone; bytes == 0: not served
constexpr int kNmsBatchMaxDet = 2048;                                          // the kept list lives in LDS
struct NmsBatchLayout { int P; size_t off_count, off_keep, off_keys, off_stage, bytes; };   // P: key slots per image (cap rounded up to a power of two)
NmsBatchLayout nms_batch_layout(int B, int cap, int max_det);
hipError_t launch_nms_batch(const adayolo_nms_batch_args& a, hipStream_t s);

}  // namespace adayolo
