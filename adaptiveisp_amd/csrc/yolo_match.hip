// Detection / label matching of the eval harness for a whole batch in ONE launch (adayolo_match, include/adayolo.h): what
// val/harness.py does per image with scale_boxes twice, process_batch (val/metrics.py, ~40 small launches) and the confusion
// matrix (val/metrics.py: ConfusionMatrix.process_batch) — the post-NMS detections and the targets mapped to native image space,
// the `correct` matrix at every IoU level, the confusion counts added on the device.
//
// One workgroup per image. The rules are two bipartite arg-maxes each:
//   correct    a detection claims the SAME-CLASS label it has the highest IoU with (lowest label index on equal IoUs) at every
//              level its IoU reaches; per level a label credits the claimant with the lowest detection index;
//   confusion  a detection with conf > cm_conf claims the label of ANY class it has the highest IoU with if that IoU is > cm_iou;
//              a label credits the claimant with the highest IoU (then the lowest detection index).
// The state lives on the LABEL side, in LDS: per label and level the lowest claiming detection (atomicMin), per label the best
// claimant as one 64-bit key (IoU bits, inverted detection index: atomicMax). Detections keep nothing between passes — one per
// thread, its best labels in registers while the labels stream through LDS — so neither count is capped:
//   * labels are taken kLabelChunk at a time: the image's rows are gathered from `targets` in row order (a ballot prefix sum
//     compacts them; the rows of an image need not be contiguous) and mapped to native space on the way in;
//   * with more than one chunk, the chunk whose state is being built stays fixed while every detection walks ALL chunks again for
//     its arg-max (the labels are re-gathered: M^2 / kLabelChunk label loads per detection instead of M — images with more than
//     kLabelChunk labels pay for it, nobody else does); detections beyond kThreads are further rounds of the same loop.
// When a chunk's state is complete, its labels write the results: correct[first claimant][level] = 1 (the rows were zeroed
// first), confusion[det class][label class] += 1 or confusion[nc][label class] += 1. "Every kept detection that was not credited
// is a background prediction, provided the image has a claim at all" is done without a per-detection flag: a credit also takes
// one from confusion[det class][nc], and at the end every kept detection adds one there — integer atomics commute, so the
// caller's buffer holds exact sums once the launch is done.
//
// fp32 arithmetic is the host path's, operation for operation (boxes.py: scale_boxes / clip_boxes / xywh2xyxy, metrics.py:
// box_iou): (x - pad) / gain then the clamp; (rb - lt) clamped at 0 before the product; inter / (area_label + area_det - inter
// + 1e-7f). Contraction is off for this file (the library's other files keep the default), and nothing relaxes the division.
#include "yolo_internal.h"

#pragma clang fp contract(off)

namespace adayolo {

constexpr int kMatchThreads = 256;       // one detection per thread and round; tests/test_gpu_match.py sizes its cases by these two
constexpr int kLabelChunk = 256;         // labels staged in LDS at a time
constexpr int kMaxLevels = 16;           // ADAYOLO_MATCH_MAX_IOU

struct Geom { float gain, padx, pady, h0, w0; bool native; };

__device__ __forceinline__ float4 to_native(float4 b, const Geom& g) {
    if (g.native) return b;
    b.x = fminf(fmaxf((b.x - g.padx) / g.gain, 0.0f), g.w0);
    b.y = fminf(fmaxf((b.y - g.pady) / g.gain, 0.0f), g.h0);
    b.z = fminf(fmaxf((b.z - g.padx) / g.gain, 0.0f), g.w0);
    b.w = fminf(fmaxf((b.w - g.pady) / g.gain, 0.0f), g.h0);
    return b;
}

// box_iou(label, detection) of val/metrics.py
__device__ __forceinline__ float iou_label_det(const float4 l, const float4 d, float area_d) {
    const float w = fmaxf(fminf(l.z, d.z) - fmaxf(l.x, d.x), 0.0f);
    const float h = fmaxf(fminf(l.w, d.w) - fmaxf(l.y, d.y), 0.0f);
    const float inter = w * h;
    const float area_l = (l.z - l.x) * (l.w - l.y);
    return inter / (area_l + area_d - inter + 1e-7f);
}

__global__ __launch_bounds__(kMatchThreads) void k_match(const adayolo_match_args a) {
    __shared__ float4 s_box[kLabelChunk];                  // the staged chunk: native-space boxes and classes
    __shared__ float s_cls[kLabelChunk];
    __shared__ float s_state_cls[kLabelChunk];             // classes of the chunk whose state is being built
    __shared__ int s_first[kLabelChunk * kMaxLevels];      // [label][level] lowest claiming detection
    __shared__ unsigned long long s_win[kLabelChunk];      // best confusion claimant: IoU bits << 32 | ~detection
    __shared__ float s_level[kMaxLevels];
    __shared__ int s_wave[kMatchThreads / 64];
    __shared__ int s_count, s_any_claim;

    const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int T = a.n_iou, nc = a.nc, n = a.n_targets;
    const long d_lo = a.det_offset[b];
    const int N = a.det_offset[b + 1] - a.det_offset[b];
    const float image = (float)b;
    Geom g = {};
    g.native = (a.flags & ADAYOLO_MATCH_NATIVE) != 0;
    if (!g.native) {
        const float* q = a.geom + 5 * (long)b;
        g.gain = q[0]; g.padx = q[1]; g.pady = q[2]; g.h0 = q[3]; g.w0 = q[4];
    }
    if (tid < T) s_level[tid] = a.iouv[tid];
    if (tid == 0) { s_count = 0; s_any_claim = 0; }
    __syncthreads();

    // ---- the detections in native space, their `correct` rows zeroed; the number of labels of this image
    for (int d = tid; d < N; d += kMatchThreads) {
        const float* r = a.det + 6 * (d_lo + d);
        const float4 box = to_native(make_float4(r[0], r[1], r[2], r[3]), g);
        float* o = a.predn + 6 * (d_lo + d);
        o[0] = box.x; o[1] = box.y; o[2] = box.z; o[3] = box.w; o[4] = r[4]; o[5] = r[5];
    }
    for (long i = tid; i < (long)N * T; i += kMatchThreads) a.correct[d_lo * T + i] = 0;
    int mine = 0;
    for (int r = tid; r < n; r += kMatchThreads) mine += a.targets[6 * (long)r] == image;
    if (mine) atomicAdd(&s_count, mine);
    __syncthreads();
    const int M = s_count;
    const int nchunks = (M + kLabelChunk - 1) / kLabelChunk;

    // labels [c * kLabelChunk, ...) of this image, in row order, into s_box / s_cls (all threads; ends with a barrier)
    auto stage = [&](int c) {
        const int lo = c * kLabelChunk, hi = lo + kLabelChunk;
        int base = 0;
        for (int r0 = 0; r0 < n && base < hi; r0 += kMatchThreads) {
            const int r = r0 + tid;
            const float* row = a.targets + 6 * (long)r;
            const bool has = r < n && row[0] == image;
            const unsigned long long vote = __ballot(has);
            if (lane == 0) s_wave[wave] = __popcll(vote);
            __syncthreads();
            int pos = base + __popcll(vote & ((1ull << lane) - 1ull)), total = 0;
            for (int w = 0; w < kMatchThreads / 64; ++w) {
                if (w < wave) pos += s_wave[w];
                total += s_wave[w];
            }
            if (has && pos >= lo && pos < hi) {
                float4 box;
                if (g.native) {
                    box = make_float4(row[2], row[3], row[4], row[5]);
                } else {                                   // xywh2xyxy, then the same map as the detections
                    const float hw = row[4] / 2.0f, hh = row[5] / 2.0f;
                    box = to_native(make_float4(row[2] - hw, row[3] - hh, row[2] + hw, row[3] + hh), g);
                }
                s_box[pos - lo] = box;
                s_cls[pos - lo] = row[1];
            }
            __syncthreads();
            base += total;
        }
    };

    int staged = -1;
    for (int c = 0; c < nchunks; ++c) {
        const int lo = c * kLabelChunk, cnt = min(kLabelChunk, M - lo);
        if (staged != c) { stage(c); staged = c; }
        for (int i = tid; i < cnt; i += kMatchThreads) { s_state_cls[i] = s_cls[i]; s_win[i] = 0ull; }
        for (int i = tid; i < cnt * kMaxLevels; i += kMatchThreads) s_first[i] = 0x7fffffff;
        __syncthreads();
        for (int d0 = 0; d0 < N; d0 += kMatchThreads) {
            const int d = d0 + tid;
            const bool live = d < N;
            float4 box = make_float4(0.f, 0.f, 0.f, 0.f);
            float conf = 0.f, cls = -1.f;
            if (live) {
                const float* r = a.det + 6 * (d_lo + d);
                box = to_native(make_float4(r[0], r[1], r[2], r[3]), g);
                conf = r[4]; cls = r[5];
            }
            const float area = (box.z - box.x) * (box.w - box.y);
            float same_iou = -1.0f, any_iou = -1.0f;       // arg-max over the labels: same class / any class
            int same_label = 0, any_label = 0;
            for (int c2 = 0; c2 < nchunks; ++c2) {
                if (staged != c2) { __syncthreads(); stage(c2); staged = c2; }
                const int cnt2 = min(kLabelChunk, M - c2 * kLabelChunk);
                if (live) {
                    for (int j = 0; j < cnt2; ++j) {
                        const float v = iou_label_det(s_box[j], box, area);
                        if (v > any_iou) { any_iou = v; any_label = c2 * kLabelChunk + j; }
                        if (s_cls[j] == cls && v > same_iou) { same_iou = v; same_label = c2 * kLabelChunk + j; }
                    }
                }
            }
            if (live && same_label >= lo && same_label < lo + cnt) {
                for (int t = 0; t < T; ++t)
                    if (same_iou >= s_level[t]) atomicMin(&s_first[(same_label - lo) * kMaxLevels + t], d);
            }
            if (live && a.confusion && conf > a.cm_conf && any_iou > a.cm_iou && any_label >= lo && any_label < lo + cnt) {
                const unsigned long long key = ((unsigned long long)__float_as_uint(any_iou) << 32) | (0xffffffffu - (unsigned)d);
                atomicMax(&s_win[any_label - lo], key);
            }
        }
        __syncthreads();
        // ---- the chunk's labels write what their state says
        for (int i = tid; i < cnt * T; i += kMatchThreads) {
            const int l = i / T, t = i - l * T;
            const int first = s_first[l * kMaxLevels + t];
            if (first < N) a.correct[(d_lo + first) * T + t] = 1;
        }
        if (a.confusion) {
            for (int l = tid; l < cnt; l += kMatchThreads) {
                const int lc = (int)s_state_cls[l];
                const bool label_ok = (unsigned)lc < (unsigned)nc;     // a class outside [0, nc) has no row or column
                const unsigned long long key = s_win[l];
                if (key == 0ull) {
                    if (label_ok) atomicAdd(&a.confusion[nc * (nc + 1) + lc], 1);
                    continue;
                }
                s_any_claim = 1;                                       // a claim is a claim whatever the classes are
                const int d = (int)(0xffffffffu - (unsigned)(key & 0xffffffffull));
                const int dc = (int)a.det[6 * (d_lo + d) + 5];
                if ((unsigned)dc >= (unsigned)nc) continue;
                if (label_ok) atomicAdd(&a.confusion[dc * (nc + 1) + lc], 1);
                atomicAdd(&a.confusion[dc * (nc + 1) + nc], -1);       // credited: it is no background prediction, see below
            }
        }
        __syncthreads();
    }
    // ---- an image with a claim: every kept detection counts as a background prediction (the credited ones gave theirs back)
    if (a.confusion && s_any_claim) {
        for (int d = tid; d < N; d += kMatchThreads) {
            const float* r = a.det + 6 * (d_lo + d);
            const int dc = (int)r[5];
            if (r[4] > a.cm_conf && (unsigned)dc < (unsigned)nc) atomicAdd(&a.confusion[dc * (nc + 1) + nc], 1);
        }
    }
}

hipError_t launch_match(const adayolo_match_args& a, hipStream_t s) {
    hipLaunchKernelGGL(k_match, dim3(a.batch), dim3(kMatchThreads), 0, s, a);
    return hipGetLastError();
}

}  // namespace adayolo
