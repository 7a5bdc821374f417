// non_max_suppression of the eval loop for a WHOLE batch on the device (adayolo_nms_batch, include/adayolo.h): from the
// detector's decoded predictions [B, N, 5+nc] to the kept rows of every image, image-major, with their row offsets — the
// inputs of adayolo_match (yolo_match.hip) — in four launches whatever B, the data or the candidate counts are, with no host
// read in between. What val/nms.py::non_max_suppression does with a dozen torch launches per batch plus an argsort, a gather,
// two NMS launches and a host read per image.
//
//   k_nmsb_init        zeroes the per-image candidate counters and status words;
//   k_nmsb_candidates  one thread per prediction row: obj > conf, then one candidate per class with obj*cls > conf
//                      (multi_label, nc > 1) or the best class (lowest index on equal products). A candidate is ONE 64-bit key,
//                      appended to its image's list through an atomic counter (one atomic per wave and image): high word = ~(score bits) (scores are positive
//                      floats, so ascending keys are descending scores), low word = row * nc + class (ascending: the host
//                      path's stable argsort over candidates in `nonzero` order). Keys are unique, so the sorted list does not
//                      depend on the order the atomics were served in. An append past `cap` sets the image's status, nothing
//                      is written, and the image gets no rows;
//   k_nmsb_image       one workgroup per image: (1) bitonic sort of the keys, padded with all-ones keys to a power of two, in
//                      tiles of kTile keys in LDS; strides of kTile and more are passes over global memory between workgroup
//                      barriers; (2) greedy NMS over the first min(count, max_nms) keys, 64 at a time: box, score and class are
//                      re-derived from the key and the prediction row; every thread tests the block against the kept list (in
//                      LDS: at most max_det boxes are ever kept), one wave builds the block's 64 x 64 suppression words, the
//                      greedy walk inside the block runs identically in every thread, the kept boxes are appended; it stops at
//                      max_det keeps. No n^2 mask;
//   k_nmsb_compact     det_offset = prefix sum of the keep counts; image b's rows move from its staging slot to
//                      det[det_offset[b] ...].
//
// fp32 arithmetic is the host path's, operation for operation: score = cls * obj; xyxy = (x - w/2, y - h/2, x + w/2, y + h/2);
// class offset = cls * 7680 (0 with `agnostic`) added to the four coordinates; box_iou_tv > iou_thres. Contraction is off for
// this file (the library's other files keep the default), including the shared IoU header below.
#pragma clang fp contract(off)
#include "yolo_internal.h"
#include "yolo_nms_iou.h"

namespace adayolo {

constexpr int kNmsbThreads = 1024;       // k_nmsb_image: 16 waves
constexpr int kTile = 4096;              // keys sorted in LDS at a time (32 KiB); kNmsBatchMaxDet float4 fit the same bytes
constexpr float kMaxWh = 7680.0f;        // class offset in pixels (val/nms.py: MAX_WH)
static_assert(kNmsBatchMaxDet * sizeof(float4) <= kTile * sizeof(unsigned long long), "the kept list reuses the sort tile");

NmsBatchLayout nms_batch_layout(int B, int cap, int max_det) {
    NmsBatchLayout L = {};
    if (B < 0 || cap < 1 || cap > (1 << 30) || max_det < 1) return L;
    int P = 1;
    while (P < cap) P <<= 1;
    const size_t a = 256;
    L.P = P;
    L.off_count = 0;                                                     // int [B] candidates appended (may exceed cap)
    L.off_keep = (size_t)B * 4;                                          // int [B] rows kept
    L.off_keys = ((size_t)B * 8 + a - 1) / a * a;                        // u64 [B][P]
    L.off_stage = L.off_keys + (size_t)B * P * 8;                        // float [B][max_det][6]
    L.bytes = L.off_stage + ((size_t)B * max_det * 24 + a - 1) / a * a;
    return L;
}

struct NmsbArgs {
    const float* pred; long stride;
    int B, N, nc, cap, max_nms, max_det, P;
    float conf, thr;
    bool multi, agnostic;
    int* count; int* keep; unsigned long long* keys; float* stage;
    float* det; int* det_offset; int* status;
};

__global__ void k_nmsb_init(int B, int* __restrict__ count, int* __restrict__ status) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < B) { count[i] = 0; status[i] = 0; }
}

// Append the candidates of a wave's lanes (every lane of the wave calls this together; `pass`: this lane has one). One atomic per
// wave and image instead of one per candidate: at conf 0.001 nearly every (row, class) of an untrained detector passes, and a
// million atomics on one counter take longer than everything else in the call. The slot a key lands in does not matter.
__device__ __forceinline__ void nmsb_append(const NmsbArgs& a, bool pass, int b, float score, unsigned idx) {
    const int lane = threadIdx.x & 63;
    unsigned long long todo = __ballot(pass);
    while (todo) {                                                       // wave-uniform: one round per image among the lanes
        const int leader = __builtin_ctzll(todo);
        const int lb = __shfl(b, leader);
        const bool mine = pass && b == lb;
        const unsigned long long grp = __ballot(mine);
        todo &= ~grp;
        int base = 0;
        if (lane == leader) base = atomicAdd(&a.count[lb], __popcll(grp));
        base = __shfl(base, leader);
        if (mine) {
            const int pos = base + __popcll(grp & ((1ull << lane) - 1ull));
            if (pos < a.cap)
                a.keys[(size_t)b * a.P + pos] = ((unsigned long long)(~__float_as_uint(score)) << 32) | idx;
            else
                a.status[b] = ADAYOLO_NMS_OVERFLOW;
        }
    }
}

__global__ __launch_bounds__(256) void k_nmsb_candidates(const NmsbArgs a) {
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    const bool valid = i < (long)a.B * a.N;                              // no early return: the appends are wave-wide
    const int b = valid ? (int)(i / a.N) : 0, row = valid ? (int)(i - (long)b * a.N) : 0;
    const float* p = a.pred + (valid ? i : 0) * a.stride;
    const float obj = p[4];
    const bool cand = valid && obj > a.conf;
    if (a.multi) {
        for (int c = 0; c < a.nc; ++c) {
            const float s = p[5 + c] * obj;
            nmsb_append(a, cand && s > a.conf, b, s, (unsigned)row * a.nc + c);
        }
    } else {
        float best = p[5] * obj;
        int bc = 0;
        for (int c = 1; c < a.nc; ++c) {
            const float s = p[5 + c] * obj;
            if (s > best) { best = s; bc = c; }
        }
        nmsb_append(a, cand && best > a.conf, b, best, (unsigned)row * a.nc + bc);
    }
}

// one compare-exchange of the bitonic network: positions i < l, ascending when `up`
__device__ __forceinline__ void cmpx(unsigned long long& x, unsigned long long& y, bool up) {
    if ((x > y) == up) { const unsigned long long t = x; x = y; y = t; }
}

__global__ __launch_bounds__(kNmsbThreads) void k_nmsb_image(const NmsbArgs a) {
    __shared__ __attribute__((aligned(16))) unsigned long long s_tile[kTile];   // the sort's tile, then the kept boxes
    __shared__ float4 s_box[64];                     // the block's boxes, class offset added
    __shared__ float s_row[64 * 6];                  // ... and their output rows
    __shared__ unsigned long long s_diag[64];        // which later boxes of the block does box r suppress
    __shared__ unsigned long long s_sup;             // boxes of the block suppressed by the kept list

    const int b = blockIdx.x, tid = threadIdx.x;
    unsigned long long* const keys = a.keys + (size_t)b * a.P;
    if (a.count[b] > a.cap) {                        // overflowed (uniform over the workgroup): its rows would be unusable — none
        if (tid == 0) a.keep[b] = 0;
        return;
    }
    const int n = a.count[b];
    int P = 1;
    while (P < n) P <<= 1;                           // <= a.P: n <= cap
    for (int i = n + tid; i < P; i += kNmsbThreads) keys[i] = ~0ull;
    __syncthreads();

    // ---- (1) bitonic sort of keys[0, P), ascending
    const int tile_n = min(P, kTile);
    // the passes with stride < tile_n of stages k_from .. k_to, tile by tile in LDS
    auto local = [&](int k_from, int k_to) {
        for (int t0 = 0; t0 < P; t0 += tile_n) {
            for (int i = tid; i < tile_n; i += kNmsbThreads) s_tile[i] = keys[t0 + i];
            __syncthreads();
            for (int k = k_from; k <= k_to; k <<= 1) {
                for (int j = min(k >> 1, tile_n >> 1); j > 0; j >>= 1) {
                    for (int q = tid; q < (tile_n >> 1); q += kNmsbThreads) {
                        const int i = ((q & ~(j - 1)) << 1) | (q & (j - 1)), l = i | j;
                        cmpx(s_tile[i], s_tile[l], ((t0 + i) & k) == 0);
                    }
                    __syncthreads();
                }
            }
            for (int i = tid; i < tile_n; i += kNmsbThreads) keys[t0 + i] = s_tile[i];
            __syncthreads();
        }
    };
    if (P > 1) local(2, tile_n);
    for (int k = tile_n << 1; k <= P; k <<= 1) {
        for (int j = k >> 1; j >= tile_n; j >>= 1) {
            for (int q = tid; q < (P >> 1); q += kNmsbThreads) {
                const int i = ((q & ~(j - 1)) << 1) | (q & (j - 1)), l = i | j;
                unsigned long long x = keys[i], y = keys[l];
                const unsigned long long x0 = x;
                cmpx(x, y, (i & k) == 0);
                if (x != x0) { keys[i] = x; keys[l] = y; }
            }
            __syncthreads();
        }
        local(k, k);
    }

    // ---- (2) greedy NMS over the first m keys
    float4* const s_kept = reinterpret_cast<float4*>(s_tile);
    float* const stage = a.stage + (size_t)b * a.max_det * 6;
    const int m = min(n, a.max_nms);
    int kept = 0;
    for (int base = 0; base < m && kept < a.max_det; base += 64) {
        const int nv = min(64, m - base);
        if (tid < nv) {
            const unsigned long long key = keys[base + tid];
            const unsigned idx = (unsigned)(key & 0xffffffffull);
            const int row = (int)(idx / (unsigned)a.nc), c = (int)(idx - (unsigned)row * a.nc);
            const float* p = a.pred + ((long)b * a.N + row) * a.stride;
            const float hw = p[2] / 2.0f, hh = p[3] / 2.0f;
            const float4 box = make_float4(p[0] - hw, p[1] - hh, p[0] + hw, p[1] + hh);
            const float cls = (float)c;
            const float off = cls * (a.agnostic ? 0.0f : kMaxWh);
            s_box[tid] = make_float4(box.x + off, box.y + off, box.z + off, box.w + off);
            float* o = s_row + tid * 6;
            o[0] = box.x; o[1] = box.y; o[2] = box.z; o[3] = box.w;
            o[4] = __uint_as_float(~(unsigned)(key >> 32));            // the product the candidate pass computed
            o[5] = cls;
        }
        if (tid == 0) s_sup = 0ull;
        __syncthreads();
        {   // the block against the kept list: thread -> (box of the block, every 16th kept box)
            const int c = tid & 63;
            if (c < nv) {
                const float4 me = s_box[c];
                bool sup = false;
                for (int k = tid >> 6; k < kept && !sup; k += kNmsbThreads / 64) sup = box_iou_tv(s_kept[k], me) > a.thr;
                if (sup) atomicOr(&s_sup, 1ull << c);
            }
        }
        if (tid < 64) {                                                // the block against itself
            unsigned long long bits = 0ull;
            if (tid < nv) {
                const float4 me = s_box[tid];
                for (int j = tid + 1; j < nv; ++j)
                    if (box_iou_tv(me, s_box[j]) > a.thr) bits |= 1ull << j;
            }
            s_diag[tid] = bits;
        }
        __syncthreads();
        // the greedy walk inside the block, identically in every thread
        unsigned long long cur = s_sup, keptmask = 0ull;
        int cnt = kept;
        for (int r = 0; r < nv && cnt < a.max_det; ++r) {
            if (!((cur >> r) & 1ull)) {
                keptmask |= 1ull << r;
                cur |= s_diag[r];
                ++cnt;
            }
        }
        __syncthreads();                                               // everyone has read s_sup / s_diag / s_kept
        if (tid < nv && ((keptmask >> tid) & 1ull)) {
            const int pos = kept + __popcll(keptmask & ((1ull << tid) - 1ull));   // < max_det
            s_kept[pos] = s_box[tid];
            for (int e = 0; e < 6; ++e) stage[pos * 6 + e] = s_row[tid * 6 + e];
        }
        kept = cnt;
        __syncthreads();
    }
    if (tid == 0) a.keep[b] = kept;
}

__global__ __launch_bounds__(256) void k_nmsb_compact(const NmsbArgs a) {
    const int b = blockIdx.x, tid = threadIdx.x;
    int lo = 0;
    for (int i = 0; i < b; ++i) lo += a.keep[i];
    const int k = a.keep[b];
    if (tid == 0) {
        a.det_offset[b + 1] = lo + k;
        if (b == 0) a.det_offset[0] = 0;
    }
    const float* src = a.stage + (size_t)b * a.max_det * 6;
    float* dst = a.det + (size_t)lo * 6;
    for (int i = tid; i < k * 6; i += 256) dst[i] = src[i];
}

hipError_t launch_nms_batch(const adayolo_nms_batch_args& g, hipStream_t s) {
    const NmsBatchLayout L = nms_batch_layout(g.B, g.cap, g.max_det);
    unsigned char* ws = static_cast<unsigned char*>(g.workspace);
    NmsbArgs a = {};
    a.pred = g.pred; a.stride = g.pred_row_stride;
    a.B = g.B; a.N = g.N; a.nc = g.nc; a.cap = g.cap; a.max_nms = g.max_nms; a.max_det = g.max_det; a.P = L.P;
    a.conf = g.conf_thres; a.thr = g.iou_thres;
    a.multi = (g.flags & ADAYOLO_NMS_MULTI_LABEL) && g.nc > 1;
    a.agnostic = (g.flags & ADAYOLO_NMS_AGNOSTIC) != 0;
    a.count = reinterpret_cast<int*>(ws + L.off_count);
    a.keep = reinterpret_cast<int*>(ws + L.off_keep);
    a.keys = reinterpret_cast<unsigned long long*>(ws + L.off_keys);
    a.stage = reinterpret_cast<float*>(ws + L.off_stage);
    a.det = g.det; a.det_offset = g.det_offset; a.status = g.status;
    const long rows = (long)g.B * g.N;
    hipLaunchKernelGGL(k_nmsb_init, dim3((g.B + 255) / 256), dim3(256), 0, s, g.B, a.count, a.status);
    hipLaunchKernelGGL(k_nmsb_candidates, dim3((unsigned)((rows + 255) / 256)), dim3(256), 0, s, a);
    hipLaunchKernelGGL(k_nmsb_image, dim3(g.B), dim3(kNmsbThreads), 0, s, a);
    hipLaunchKernelGGL(k_nmsb_compact, dim3(g.B), dim3(256), 0, s, a);
    return hipGetLastError();
}

}  // namespace adayolo
