// Image export (include/adaisp.h, adaisp_export_u8): planar fp32 RGB [B,3,H,W] -> interleaved uint8 BGR [B,H,W,3], the
// bytes the reference's `save_img` (util.py:21-40) hands to cv2.imwrite after OpenCV's float -> 8U conversion:
//
//   x = isnan(x) ? 0 : x;  x = clip(x, 0, 1);  y = x * 255.0f (fp32);  u8 = saturate_cast<uchar>(y) = round half to even
//
// Mapping: a lane owns 4 consecutive pixels of one image. With H*W % 4 == 0 and a 16-byte aligned `img` every plane row of
// 4 starts 16-byte aligned: three 16-byte loads (R, G, B), and the 12 output bytes go out as three 4-byte stores when `out`
// is 4-byte aligned (H*W % 4 == 0 keeps every lane's 12-byte group at a multiple of 4). Any other alignment or size takes
// the scalar path: 4-byte loads and byte stores, each pixel bounds-checked. Nothing is written past B*H*W*3 bytes.
#include "isp_internal.h"

namespace adaisp {
namespace {

constexpr int EXP_THREADS = 256;

__device__ __forceinline__ uint32_t to_u8(float x) {
    x = (x != x) ? 0.0f : x;                                   // img[np.isnan(img)] = 0
    x = fminf(fmaxf(x, 0.0f), 1.0f);                           // np.clip(img, 0, 1)
    const float y = x * 255.0f;                                // img * 255.0 (float32 array times a Python float)
    return (uint32_t)__float2int_rn(y);                        // cvRound: nearest, ties to even; y is in [0, 255]
}

template <bool VEC>
__global__ __launch_bounds__(EXP_THREADS) void k_export_u8(const float* __restrict__ img, uint8_t* __restrict__ out,
                                                           long hw) {
    const int b = blockIdx.y;
    const long p0 = ((long)blockIdx.x * EXP_THREADS + threadIdx.x) * 4;
    if (p0 >= hw) return;
    const float* __restrict__ r = img + (long)b * 3 * hw;
    const float* __restrict__ g = r + hw;
    const float* __restrict__ bl = g + hw;
    uint8_t* __restrict__ dst = out + ((long)b * hw + p0) * 3;
    if (VEC) {
        const float4 R = *reinterpret_cast<const float4*>(r + p0);
        const float4 G = *reinterpret_cast<const float4*>(g + p0);
        const float4 B = *reinterpret_cast<const float4*>(bl + p0);
        // bytes in memory order: B0 G0 R0 B1 | G1 R1 B2 G2 | R2 B3 G3 R3
        const uint32_t w0 = to_u8(B.x) | to_u8(G.x) << 8 | to_u8(R.x) << 16 | to_u8(B.y) << 24;
        const uint32_t w1 = to_u8(G.y) | to_u8(R.y) << 8 | to_u8(B.z) << 16 | to_u8(G.z) << 24;
        const uint32_t w2 = to_u8(R.z) | to_u8(B.w) << 8 | to_u8(G.w) << 16 | to_u8(R.w) << 24;
        uint32_t* __restrict__ d = reinterpret_cast<uint32_t*>(dst);
        d[0] = w0;
        d[1] = w1;
        d[2] = w2;
    } else {
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const long p = p0 + k;
            if (p < hw) {
                dst[3 * k + 0] = (uint8_t)to_u8(bl[p]);
                dst[3 * k + 1] = (uint8_t)to_u8(g[p]);
                dst[3 * k + 2] = (uint8_t)to_u8(r[p]);
            }
        }
    }
}

}  // namespace
}  // namespace adaisp

extern "C" int adaisp_export_u8(const float* img, uint8_t* out, int B, int H, int W, void* stream) {
    using namespace adaisp;
    if (!img || !out || B <= 0 || H <= 0 || W <= 0) return ADAISP_EINVAL;
    const long hw = (long)H * W;
    const long groups = (hw + 4 * EXP_THREADS - 1) / (4 * EXP_THREADS);
    if (B > 65535 || groups > 0x7fffffffL) return ADAISP_ESHAPE;                 // grid.y; grid.x
    const bool vec = hw % 4 == 0 && reinterpret_cast<uintptr_t>(img) % 16 == 0 && reinterpret_cast<uintptr_t>(out) % 4 == 0;
    const dim3 grid((unsigned)groups, (unsigned)B);
    hipStream_t s = static_cast<hipStream_t>(stream);
    if (vec)
        hipLaunchKernelGGL((k_export_u8<true>), grid, dim3(EXP_THREADS), 0, s, img, out, hw);
    else
        hipLaunchKernelGGL((k_export_u8<false>), grid, dim3(EXP_THREADS), 0, s, img, out, hw);
    return hipGetLastError() == hipSuccess ? ADAISP_OK : ADAISP_ELAUNCH;
}
