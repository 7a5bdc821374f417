// Conv + bias + SiLU (+ residual), 256 px x 256 ch tile: the launch-per-layer kernels and launchers of the tile body in
// yolo_tile_pp.h (the persistent chain, yolo_conv_chain.hip, runs the same body).
#include "yolo_tile_pp.h"

namespace adayolo {
namespace pp {

template <int ABL, bool FUSE>
__global__ __launch_bounds__(512) void k_conv_pp(const ConvArgs a) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    ChainCtx none{nullptr, -1};
    conv_tile<ABL, FUSE, false>(a, xcd_remap(blockIdx.x, a.mtiles * a.ntiles), smem, none);
}

// the same kernel with the k-loop on v_mfma_f32_16x16x32_bf16 (MS 16)
template <int ABL, bool FUSE>
__global__ __launch_bounds__(512) void k_conv_pp_m16(const ConvArgs a) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    ChainCtx none{nullptr, -1};
    conv_tile<ABL, FUSE, false, 16>(a, xcd_remap(blockIdx.x, a.mtiles * a.ntiles), smem, none);
}

template <int ABL, bool FUSE = false, int MS = 32>
static hipError_t launch(ConvArgs a, hipStream_t s) {
    static_assert(kSmem <= 160 * 1024, "LDS budget");
    a.mtiles = (a.M + BM - 1) / BM;
    a.ntiles = a.Cout / BN;
    if constexpr (MS == 16) return launch_lds<k_conv_pp_m16<ABL, FUSE>>(dim3(a.mtiles * a.ntiles), dim3(512), kSmem, s, a);
    else return launch_lds<k_conv_pp<ABL, FUSE>>(dim3(a.mtiles * a.ntiles), dim3(512), kSmem, s, a);
}

}  // namespace pp

// variant 50 = the kernel; with -DADAYOLO_MEASURE 51..57 = the measurement builds (ABL above). hipErrorInvalidValue ->
// the shape is not served (the caller falls back to the default kernel).
hipError_t launch_conv_pp(ConvArgs a, hipStream_t s, int variant) {
    if (a.Cin % 64 || a.Cout % 256) return hipErrorInvalidValue;
    const bool m16 = mfma_shape(kShapePp) == 16;         // read at enqueue time: a captured graph keeps what it captured
#ifdef ADAYOLO_MEASURE
    if (m16) {
        if (variant == 56) return pp::launch<6, false, 16>(a, s);
        if (variant == 57) return pp::launch<7, false, 16>(a, s);
    }
    if (variant == 51) return pp::launch<1>(a, s);
    if (variant == 52) return pp::launch<2>(a, s);
    if (variant == 53) return pp::launch<3>(a, s);
    if (variant == 54) return pp::launch<4>(a, s);
    if (variant == 55) return pp::launch<5>(a, s);
    if (variant == 56) return pp::launch<6>(a, s);
    if (variant == 57) return pp::launch<7>(a, s);
    if (variant == 58) return pp::launch<8>(a, s);
    if (variant == 59) return pp::launch<9>(a, s);
#endif
    (void)variant;
    if (a.w2) {                                          // fused 1x1 second layer: the tile must hold all channels
        if (a.Cout != 256 || !a.bias2 || !a.out2) return hipErrorInvalidValue;
#ifdef ADAYOLO_MEASURE
        if (getenv("ADAYOLO_PP_STAMPS")) return m16 ? pp::launch<7, true, 16>(a, s) : pp::launch<7, true>(a, s);
#endif
        return m16 ? pp::launch<0, true, 16>(a, s) : pp::launch<0, true>(a, s);
    }
    return m16 ? pp::launch<0, false, 16>(a, s) : pp::launch<0>(a, s);
}

#ifdef ADAYOLO_MEASURE
// measurement helper (not part of the ABI): copies the stamps of the last variant-57 launch
extern "C" int adayolo_debug_stamps(unsigned long long* dst, int n) {
    return hipMemcpyFromSymbol(dst, HIP_SYMBOL(pp::g_stamp), sizeof(unsigned long long) * n) == hipSuccess ? 0 : -1;
}
#endif

}  // namespace adayolo
