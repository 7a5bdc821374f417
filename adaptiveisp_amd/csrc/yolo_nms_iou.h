// The IoU of greedy NMS (torchvision.ops.nms's published arithmetic, restated by the CPU oracle): shared by the per-image
// kernels (yolo_nms.hip) and the whole-batch path (yolo_nms_batch.hip). Floating-point contraction is the including file's
// choice: yolo_nms_batch.hip turns it off before this header, because its results are held to the host path without tolerance.
#pragma once
#include <hip/hip_runtime.h>

namespace adayolo {

__device__ __forceinline__ float box_iou_tv(const float4 a, const float4 b) {
    const float area_a = (a.z - a.x) * (a.w - a.y), area_b = (b.z - b.x) * (b.w - b.y);
    const float w = fmaxf(fminf(a.z, b.z) - fmaxf(a.x, b.x), 0.0f);
    const float h = fmaxf(fminf(a.w, b.w) - fmaxf(a.y, b.y), 0.0f);
    const float inter = w * h;
    return inter / (area_a + area_b - inter);
}

}  // namespace adayolo
