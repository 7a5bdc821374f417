// Conv + bias + SiLU (+ residual), 256 px x 128 ch tile: the launch-per-layer kernels (plain and split-K) and launchers of the
// tile body in yolo_tile_pp128.h (the persistent chain, yolo_conv_chain.hip, runs the same body).
#include "yolo_tile_pp128.h"

namespace adayolo {
namespace pp128 {

template <int ABL, bool SPLIT>
__global__ __launch_bounds__(512) void k_conv_pp128(const ConvArgs a) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    ChainCtx none{nullptr, -1};
    const int ntile = a.mtiles * a.ntiles;
    conv_tile<ABL, SPLIT, false>(a, xcd_remap(blockIdx.x, SPLIT ? ntile * a.ksplit : ntile), smem, none);
}

// the same kernel with the k-loop on v_mfma_f32_16x16x32_bf16 (MS 16)
template <int ABL, bool SPLIT>
__global__ __launch_bounds__(512) void k_conv_pp128_m16(const ConvArgs a) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    ChainCtx none{nullptr, -1};
    const int ntile = a.mtiles * a.ntiles;
    conv_tile<ABL, SPLIT, false, 16>(a, xcd_remap(blockIdx.x, SPLIT ? ntile * a.ksplit : ntile), smem, none);
}

template <int ABL, bool SPLIT = false, int MS = 32>
static hipError_t launch(ConvArgs a, hipStream_t s) {
    static_assert(kSmem <= 160 * 1024, "LDS budget");
    a.mtiles = (a.M + BM - 1) / BM;
    a.ntiles = a.Cout / BN;
    const dim3 grid(a.mtiles * a.ntiles * (SPLIT ? a.ksplit : 1));
    if constexpr (MS == 16) return launch_lds<k_conv_pp128_m16<ABL, SPLIT>>(grid, dim3(512), kSmem, s, a);
    else return launch_lds<k_conv_pp128<ABL, SPLIT>>(grid, dim3(512), kSmem, s, a);
}

}  // namespace pp128

// Split-K form: S ranges of k-tiles per output tile. Served when the k-tiles divide evenly into ranges of at least
// kMinRange, and the tile count leaves CUs free (otherwise the plain kernel is the better one anyway). Returns the bytes of
// workspace the launch needs (tickets, then S fp32 partial tiles per output tile), 0 = not served.
size_t conv_pp128_splitk_bytes(const ConvArgs& a, int S) {
    constexpr int kMinRange = 4;
    if (a.Cin % 64 || a.Cout % 128 || S < 2 || S > 16) return 0;
    const int nK = a.ks * a.ks * (a.Cin / pp128::BK);
    if (nK % S || nK / S < kMinRange) return 0;
    const long tiles = (long)((a.M + pp128::BM - 1) / pp128::BM) * (a.Cout / pp128::BN);
    if (tiles * S > 512) return 0;
    return (size_t)((tiles * 4 + 1023) / 1024 * 1024) + (size_t)tiles * S * (pp128::BM * pp128::BN * 4);
}

hipError_t launch_conv_pp128_splitk(ConvArgs a, hipStream_t s, int S, void* workspace, size_t workspace_bytes) {
    const size_t need = conv_pp128_splitk_bytes(a, S);
    if (need == 0 || !workspace || workspace_bytes < need) return hipErrorInvalidValue;
    const long tiles = (long)((a.M + pp128::BM - 1) / pp128::BM) * (a.Cout / pp128::BN);
    a.ksplit = S;
    a.tickets = static_cast<int*>(workspace);
    a.partial = reinterpret_cast<float*>(static_cast<unsigned char*>(workspace) + (tiles * 4 + 1023) / 1024 * 1024);
    return mfma_shape(kShapePp128) == 16 ? pp128::launch<0, true, 16>(a, s) : pp128::launch<0, true>(a, s);
}

// variant 60 = the kernel; with -DADAYOLO_MEASURE 65 / 66 = measurement builds. hipErrorInvalidValue -> not served.
hipError_t launch_conv_pp128(ConvArgs a, hipStream_t s, int variant) {
    if (a.Cin % 64 || a.Cout % 128) return hipErrorInvalidValue;
    const bool m16 = mfma_shape(kShapePp128) == 16;      // read at enqueue time: a captured graph keeps what it captured
#ifdef ADAYOLO_MEASURE
    if (m16 && variant == 66) return pp128::launch<6, false, 16>(a, s);
    if (variant == 65) return pp128::launch<5>(a, s);
    if (variant == 66) return pp128::launch<6>(a, s);
    if (variant == 67) return pp128::launch<7>(a, s);
#endif
    (void)variant;
    return m16 ? pp128::launch<0, false, 16>(a, s) : pp128::launch<0>(a, s);
}

}  // namespace adayolo
