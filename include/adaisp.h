/*
 * adaisp.h — C-ABI of the MI355X-native AdaptiveISP filter stack (libadaisp.so).
 *
 * This is the drop-in boundary for the ISP hot path. The reference has no FFI of its own: its
 * boundary is the Python class API (`Filter.process(img, param)`, `Filter.forward`,
 * `Agent.forward`). Each entry point below cites the reference call it replaces
 * (paths relative to the reference checkout).
 *
 * Conventions
 *   - every pointer is a DEVICE pointer owned by the caller, fp32, contiguous;
 *   - images are planar CHW:  img[b][c][y][x],  c in {R,G,B},  shape [B,3,H,W];
 *   - params are the REGRESSED filter parameters (after tanh_range / sigmoid / exp),
 *     one row of `param_stride` floats per image;
 *   - work is enqueued on `stream` (a hipStream_t passed as void*; NULL = default stream);
 *     no call allocates, synchronises, or keeps global mutable state — all are re-entrant;
 *   - return 0 on success, a negative ADAISP_E* code otherwise (adaisp_strerror() names it).
 */
#ifndef ADAISP_H_
#define ADAISP_H_

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define ADAISP_ABI_VERSION 9

/* Kernel op codes. 0..9 follow the reference's default filter order (config.py:19-22). */
enum adaisp_op {
    ADAISP_OP_ZERO       = -1, /* all-zero one-hot: reference pdf_sample u==0 edge, agent.py:12-16,154 */
    ADAISP_OP_EXPOSURE   = 0,  /* ExposureFilter.process               isp/filters.py:223-224  n=1  */
    ADAISP_OP_GAMMA      = 1,  /* GammaFilter.process                  isp/filters.py:244-245  n=1  */
    ADAISP_OP_CCM        = 2,  /* CCMFilter.process                    isp/filters.py:703-708  n=9  */
    ADAISP_OP_SHARPEN    = 3,  /* SharpenFilter / adjust_sharpness     isp/sharpen.py:105-142  n=1  */
    ADAISP_OP_NLM        = 4,  /* DenoiseFilter / NonLocalMeansGray    isp/denoise.py:93-119   n=1  */
    ADAISP_OP_TONE       = 5,  /* ToneFilter.process                   isp/filters.py:337-347  n=8  */
    ADAISP_OP_CONTRAST   = 6,  /* ContrastFilter.process               isp/filters.py:415-419  n=1  */
    ADAISP_OP_SATPLUS    = 7,  /* SaturationPlusFilter.process         isp/filters.py:546-560  n=1  */
    ADAISP_OP_WNB        = 8,  /* WNBFilter.process                    isp/filters.py:435-437  n=1  */
    ADAISP_OP_WB         = 9,  /* ImprovedWhiteBalanceFilter.process   isp/filters.py:271-272  n=3  */
    ADAISP_OP_USM        = 10, /* SharpenUSMFilter / unsharp_mask      isp/sharpen.py:84-102   n=2  */
    ADAISP_OP_SHARPEN_V2 = 11, /* SharpenFilterV2 / sharpness          isp/sharpen.py:145-182  n=1  */
    ADAISP_OP_COLOR      = 12, /* ColorFilter.process                  isp/filters.py:293-303  n=24 */
    ADAISP_OP_COUNT      = 13
};

#define ADAISP_MAX_PARAMS 24

/* flags */
#define ADAISP_CLIP01 1u /* clamp the result to [0,1]: Filter.forward's final clip, isp/filters.py:125 */
#define ADAISP_NLM_EXACT 2u /* NLM: add the 25 patch terms in the reference's single running-sum order
                               (isp/denoise.py:60-63) instead of the default 5x5 separable association; ~3.5x slower */
#define ADAISP_NLM_SEP_V1 4u /* NLM: the compiler-scheduled form of the separable kernel (measurement / cross-check) */
#define ADAISP_NO_USM 8u /* adaisp_forward: no image of the batch selects ADAISP_OP_USM (saves its empty launch) */
#define ADAISP_NLM_TILE32 16u /* NLM: the 32-row tile of the default kernel (2 workgroups per CU) instead of the 24-row
                                 one (3 per CU); same arithmetic, same results (measurement / cross-check) */

/* error codes */
#define ADAISP_OK          0
#define ADAISP_EINVAL     -1 /* null pointer / non-positive size / bad stride  */
#define ADAISP_EOP        -2 /* unknown op code (host-known op only)           */
#define ADAISP_EALIAS     -3 /* out aliases img for a stencil op               */
#define ADAISP_ESHAPE     -4 /* shape unsupported by the op (e.g. 3x3 on H<3)  */
#define ADAISP_ELAUNCH    -5 /* hipLaunchKernel failed                         */

/*
 * One RL step of the ISP: image b is filtered by op filter_id[b] with params[b].
 * Replaces the reference's "run all filters, stack, one-hot select" of Agent.forward
 * (agent.py:103-116,154) — only the selected filter is computed.
 * `filter_id` lives on the device (no host sync is needed to pick the work); -1 — and any id outside enum adaisp_op —
 * writes zeros (the reference's all-zero one-hot row).
 * If `pooled64_next` != NULL it receives AdaptiveAvgPool2d((64,64)) of `out`
 * ([B,3,64,64]; agent.py:97 / value.py:63) for the next step's policy input — from the SAME launch for the pointwise
 * and 3x3 / 5x5 stencil ops (the kernels are cut along the pool windows; rows 16-byte aligned, H, W >= 64, pool columns
 * <= 64 px wide), bit-identical to adaisp_pool64(out); NLM images and other geometries take a pooling launch.
 * `out` must not alias `img`.
 */
int adaisp_forward(const float* img, float* out, float* pooled64_next,
                   const int32_t* filter_id, const float* params, int param_stride,
                   int B, int H, int W, unsigned flags, void* stream);

/*
 * adaisp_forward when the HOST knows the op of the step (teacher-forced schedules, `selected_filter_id` of
 * Agent.forward, agent.py:88,150-153): one op for the whole batch, per-image params, optional fused pooling. Exactly one
 * kernel is enqueued (two for NLM with pooling) instead of one per kernel family. Same results as adaisp_forward with
 * filter_id[b] == op.
 */
int adaisp_forward_uniform(int op, const float* img, float* out, float* pooled64_next,
                           const float* params, int param_stride,
                           int B, int H, int W, unsigned flags, void* stream);

/*
 * Same arithmetic with ONE host-known op for the whole batch: Filter.process(img, param)
 * (flags = 0) and the image part of Filter.forward (flags = ADAISP_CLIP01), isp/filters.py:81,115-125.
 * Pointwise ops may run in place (out == img).
 */
int adaisp_process(int op, const float* img, float* out,
                   const float* params, int param_stride,
                   int B, int H, int W, unsigned flags, void* stream);

/*
 * Parameter gradients of adaisp_forward: grad_params[b][k] = sum_px grad_out * d out / d params[b][k]
 * through the selected filter and (if ADAISP_CLIP01) the clip. This is the only gradient the
 * reference's training needs (train.py:341-342: imgs is a constant leaf).
 * grad_params ([B,param_stride]) is zero-filled by the callee.
 */
int adaisp_backward_params(const float* img, const float* grad_out,
                           const int32_t* filter_id, const float* params, int param_stride,
                           float* grad_params,
                           int B, int H, int W, unsigned flags, void* stream);

/*
 * Image gradient of adaisp_forward: grad_img[b] = d/d img[b] of sum_px grad_out * out through the selected filter and
 * (if ADAISP_CLIP01) the clip — what the reference's autograd gives for the filter modules (isp/filters.py, isp/sharpen.py,
 * isp/denoise.py), subgradient conventions included: clamp / clip pass on the closed interval (the output clip :125, Gamma's
 * clip :245, the input clips of SaturationPlus and Denoise :547,584, the tone / colour segments :300,343 — a pixel on a
 * breakpoint takes the slope of both segments); max / min over the channels route to the first channel on ties and the hue
 * keeps the last masked write (:455-466); the 1-px frame of the 3x3 sharpen pair passes through (isp/sharpen.py:133-138);
 * USM's reflect padding folds back (:63-81); NLM wraps circularly and its relu passes nothing at a zero patch distance
 * (isp/denoise.py:103-119). Parameter gradients stay with adaisp_backward_params.
 * Every element of grad_img ([B,3,H,W]) is written; images whose op is -1 or outside enum adaisp_op get zeros. grad_img must
 * not overlap img or grad_out (ADAISP_EALIAS). Only ADAISP_CLIP01 of `flags` has a meaning. `workspace` (at least
 * adaisp_backward_image_workspace_bytes(B, H, W)) is caller-owned scratch; nothing is allocated or synchronised, so the
 * call can be captured in a hipGraph. H, W >= 3 (as adaisp_forward).
 */
size_t adaisp_backward_image_workspace_bytes(int B, int H, int W);
int adaisp_backward_image(const float* img, const float* grad_out,
                          const int32_t* filter_id, const float* params, int param_stride,
                          float* grad_img, void* workspace, size_t workspace_bytes,
                          int B, int H, int W, unsigned flags, void* stream);

/*
 * Bayer demosaic front-end — an EXTENSION (north_star's raw-Bayer entry; the reference has no demosaic, only the
 * inverse packing `mosaic` / `reconstruct_bayer`, isp/unprocess_np.py:82-128).
 * raw: uint16 [B,H,W] colour-filter-array samples; pattern = 2*ry + rx, the position of the RED sample in the 2x2
 * cell (ADAISP_CFA_RGGB 0, GRBG 1, GBRG 2, BGGR 3). out: planar fp32 [B,3,H,W], bilinear interpolation of
 * (raw - black_level) / (white_level - black_level); mirrored borders. H and W even.
 */
#define ADAISP_CFA_RGGB 0
#define ADAISP_CFA_GRBG 1
#define ADAISP_CFA_GBRG 2
#define ADAISP_CFA_BGGR 3
int adaisp_demosaic(const uint16_t* raw, float* out, int B, int H, int W, int pattern,
                    float black_level, float white_level, void* stream);

/*
 * Replay-pool input conversion: decoded images -> the [B,3,S,S] fp32 letterboxed batch the RL trainer stores
 * (the reference's `lod` and `coco` loaders, replay_memory.py:60-97).
 * src: uint8 HWC BGR pixels (cv2.imread order) of every image, packed at any byte offsets. desc: a DEVICE array of B
 * records; image b is desc[b].h x desc[b].w pixels at src + desc[b].src_offset, placed at (top, left) of its S x S
 * output; every other output sample is exactly 0 (a placement that does not fit the frame gives an all-zero image).
 *   flags 0                 convert: out = float(u8) / 255 (LoadImagesAndLabelsNormalizeReplay, dataset.py:794-897)
 *   ADAISP_UNP_UNPROCESS    unprocess_wo_mosaic, isp/unprocess_np.py:248-292 (dataset.py:458-471), in fp32, with the
 *                           per-image parameters p[] below (the random draws are the caller's)
 *   | ADAISP_UNP_NOISE      + shot / read noise, :177-181 and the clip after it. The normals come from Philox4x32-10
 *                           keyed by (seed, desc[b].serial), counter = the pixel's index in the un-padded image
 *                           (Box-Muller): they depend on (seed, serial) only, not on the batch, position or offset.
 * No allocation, no host synchronisation: capturable in a hipGraph. B <= 65535, S <= 32768.
 */
#define ADAISP_UNP_UNPROCESS 1u
#define ADAISP_UNP_NOISE 2u
#define ADAISP_UNP_CCM 0       /* p[0..8]: rgb2cam, row-major (apply_ccm: out_c = sum_k rgb2cam[c][k] in_k)      */
#define ADAISP_UNP_GAIN 9      /* p[9..11]: (1/red_gain, 1, 1/blue_gain) / rgb_gain (safe_invert_gains)          */
#define ADAISP_UNP_PRESCALE 12 /* p[12]: brightness before the inverse tone curve (the reference: 0.9)           */
#define ADAISP_UNP_RATIO 13    /* p[13]: brightness ratio after the clip (adjust_random_brightness; 1 if none)  */
#define ADAISP_UNP_SHOT 14     /* p[14], p[15]: shot and read noise (variance = x * shot + read)                 */
#define ADAISP_UNP_READ 15
typedef struct adaisp_unprocess_desc {
    int64_t src_offset;        /* byte offset of the image's first pixel in src                                  */
    int32_t h, w, top, left;   /* un-padded size and its placement in the S x S frame                            */
    uint64_t serial;           /* noise key (with the seed)                                                      */
    float p[16];               /* ADAISP_UNP_* slots (ignored by the convert mode)                               */
} adaisp_unprocess_desc;
int adaisp_unprocess(const uint8_t* src, const adaisp_unprocess_desc* desc, float* out, int B, int S,
                     uint64_t seed, unsigned flags, void* stream);

/*
 * Simulated Bayer sensor: adaisp_unprocess through a colour filter array and a quantiser, the half of the reference's
 * `unprocess` that adaisp_unprocess leaves out (`mosaic`, isp/unprocess_np.py:217-245, :82-98). src, desc, B, S, seed
 * and flags are adaisp_unprocess's. out: uint16 [B,S,S]. Inside an image's rectangle, pixel (iy, ix) in the IMAGE's
 * coordinates keeps the one channel c that `pattern` (ADAISP_CFA_*) assigns to it (the phase belongs to the image, not to
 * the frame), and stores
 *     clamp(rintf(v * (white_level - black_level)) + black_level, 0, 65535)
 * where v is exactly the fp32 value adaisp_unprocess writes for channel c of that pixel under the same flags,
 * parameters, seed and serial; with ADAISP_UNP_NOISE it carries the c-th of the pixel's three normals. Every sample
 * outside the rectangle is black_level; a placement that does not fit the frame gives an all-black image. The levels are
 * meant to be whole numbers (the conversion to uint16 drops a fraction). ADAISP_EINVAL: null pointers, bad flags,
 * unknown pattern, white_level <= black_level; ADAISP_ESHAPE: B > 65535 or S > 32768. No allocation, no host
 * synchronisation: capturable in a hipGraph.
 */
int adaisp_unprocess_bayer(const uint8_t* src, const adaisp_unprocess_desc* desc, uint16_t* out, int B, int S,
                           uint64_t seed, unsigned flags, int pattern, float black_level, float white_level,
                           void* stream);

/*
 * adaisp_demosaic's bilinear rule inside every image's own rectangle of a letterboxed plane (the output of
 * adaisp_unprocess_bayer, with the same descriptors): raw uint16 [B,S,S] -> planar fp32 [B,3,S,S]. The CFA phase is
 * relative to the rectangle's origin and the mirror (-1 -> 1, h -> h - 2) is taken at the rectangle's edges, so border
 * pixels never average with the pad and an odd top / left keeps the colours in place: inside the rectangle the output is
 * adaisp_demosaic of the crop, bit for bit (h and w may be odd: the crop continued by its mirror). Every output outside
 * the rectangle is exactly 0; an image with h < 2 or w < 2, or whose placement does not fit the frame, comes out all
 * zero. Any S >= 1. Errors and limits as adaisp_unprocess_bayer. Capturable.
 */
int adaisp_demosaic_rects(const uint16_t* raw, const adaisp_unprocess_desc* desc, float* out, int B, int S, int pattern,
                          float black_level, float white_level, void* stream);

/*
 * The two demosaics with a choice of interpolation. method ADAISP_DEMOSAIC_BILINEAR launches the kernels of adaisp_demosaic
 * / adaisp_demosaic_rects (bit-identical to them); ADAISP_DEMOSAIC_MHC is the 5 x 5 gradient-corrected linear interpolation
 * of Malvar, He and Cutler (2004), under the same contracts: raw, out, pattern, H and W even (whole frame); descriptors,
 * phase and mirror at the rectangle, exactly 0 outside it, h < 2 / w < 2 / a placement that does not fit all zero, any
 * S >= 1 (rectangles). It works on the un-normalised samples t = float(raw) - black_level. With C the centre sample, N S W E
 * the neighbours at distance 1, N2 S2 W2 E2 those at distance 2 and D = NW + NE + SW + SE:
 *     the site's own colour                                 acc = 8 C
 *     G at an R or B site                                   acc = 4 C + 2 (N + S + W + E) - (N2 + S2 + W2 + E2)
 *     R at a B site, B at an R site                         acc = 6 C + 2 D - 1.5 (N2 + S2 + W2 + E2)
 *     R or B at a G site, the wanted colour lying W / E     acc = 5 C + 4 (W + E) - D - (W2 + E2) + 0.5 (N2 + S2)
 *     R or B at a G site, the wanted colour lying N / S     acc = 5 C + 4 (N + S) - D - (N2 + S2) + 0.5 (W2 + E2)
 *     out = (acc * 0.125f) * (1.0f / (white_level - black_level))
 * With a whole-number black_level in [0, 65535] (so |raw - black_level| <= 65535) every term is a multiple of 0.5 and 2
 * |acc| <= 40 * 65535 < 2^24: acc is exact in fp32 whatever the order, the last multiply is the only rounding, and a sampled
 * colour equals the bilinear (raw - black) * inv_range bit for bit. Borders mirror without repeating the edge sample, folded
 * as often as needed (period 2n - 2, numpy's "reflect": -1 -> 1, -2 -> 2, and on a 2-pixel side -2 -> 0), which keeps the
 * Bayer phase on any side >= 2. Nothing is clamped, as in the bilinear kernels: the filters over- and undershoot at edges
 * (values outside [0,1]) and the filter stack has its own clips.
 * Arguments, limits and error codes as adaisp_demosaic / adaisp_demosaic_rects; an unknown method is ADAISP_EINVAL.
 * Other levels are accepted as they are by the bilinear entries (only white_level > black_level is checked): the filters
 * are the same, but a fractional or out-of-range black_level gives up the bit-for-bit guarantee, not the result.
 * No allocation, no host synchronisation: capturable in a hipGraph.
 */
#define ADAISP_DEMOSAIC_BILINEAR 0
#define ADAISP_DEMOSAIC_MHC      1
int adaisp_demosaic_ex(const uint16_t* raw, float* out, int B, int H, int W, int pattern, int method,
                       float black_level, float white_level, void* stream);
int adaisp_demosaic_rects_ex(const uint16_t* raw, const adaisp_unprocess_desc* desc, float* out, int B, int S,
                             int pattern, int method, float black_level, float white_level, void* stream);

/*
 * Replay-pool resampling on the device: the pixel work of `load_image` (dataloaders.py:735-750: longer side to S, area
 * filter when shrinking, bilinear otherwise) and of `letterbox`'s resize to the un-padded size (augmentations.py:111-141),
 * uint8 HWC BGR -> uint8 HWC BGR, every image with its own sizes, mode and byte offsets. Each mode reproduces the
 * project's numpy restatement of OpenCV's uint8 kernels (adaptiveisp_amd/val/loader.py) bit for bit:
 *   ADAISP_RESIZE_COPY      (W, H) == (w, h)
 *   ADAISP_RESIZE_LINEAR    resize_linear_u8: 11-bit taps, int32 horizontal pass,
 *                           (((b0 * (t >> 4)) >> 16) + ((b1 * (b >> 4)) >> 16) + 2) >> 2
 *   ADAISP_RESIZE_AREA_INT  resize_area_u8, integer factors (fx = W / w, fy = H / h): integer block sum, then
 *                           (sum + 2) >> 2 for 2 x 2 and rint(float(sum) * scale) otherwise, scale = float32(1 / (fx fy))
 *   ADAISP_RESIZE_AREA      resize_area_u8, general factors: the fp32 weights of _area_weights, horizontal pass then
 *                           vertical pass, each a sequence of one fp32 multiply then one fp32 add in source order;
 *                           round half to even, clip
 * The host builds the taps (adaptiveisp_amd/resize.py); they live in `tabs`, 32-bit words (floats by their bits):
 *   LINEAR   at tab_x: i0[w], i1[w], w0[w], w1[w] (_linear_taps); at tab_y the same over h
 *   AREA     at tab_x: ptr[w + 1], idx[nnz], weight[nnz] with nnz = ptr[w] (the nonzeros of row x of _area_weights, in
 *            source order, CSR); at tab_y the same over h
 * An image whose pixels or taps do not lie inside src_bytes / dst_bytes / tab_words, or whose mode is unknown, is not
 * written; source indices read from the taps are clamped to the image. No allocation, no host synchronisation:
 * capturable in a hipGraph. B <= 65535; max_h, max_w (the largest destination size of the batch: the grid) <= 32768.
 */
#define ADAISP_RESIZE_COPY 0
#define ADAISP_RESIZE_LINEAR 1
#define ADAISP_RESIZE_AREA_INT 2
#define ADAISP_RESIZE_AREA 3
typedef struct adaisp_resize_desc {
    int64_t src_offset;        /* byte offset of the source image's first pixel in src                           */
    int64_t dst_offset;        /* byte offset of the destination image in dst                                    */
    int64_t tab_x, tab_y;      /* word offsets of the horizontal / vertical taps in tabs (LINEAR, AREA)          */
    int32_t src_h, src_w;      /* source size                                                                    */
    int32_t dst_h, dst_w;      /* destination size                                                               */
    int32_t mode;              /* ADAISP_RESIZE_*                                                                */
    float scale;               /* AREA_INT: float32(1 / (fx * fy))                                               */
} adaisp_resize_desc;
int adaisp_resize_u8(const uint8_t* src, size_t src_bytes, uint8_t* dst, size_t dst_bytes,
                     const adaisp_resize_desc* desc, const int32_t* tabs, size_t tab_words, int B, int max_h, int max_w,
                     void* stream);

/*
 * Training augmentation of the replay-pool input, in front of adaisp_unprocess / adaisp_unprocess_bayer: the affine warp of
 * `random_perspective` (augmentations.py:144-193, perspective = 0) with the flips of dataset.py:505-514 folded into the
 * map, then the HSV tables of `augment_hsv` (augmentations.py:67-80), uint8 HWC BGR -> uint8 HWC BGR, one launch per batch.
 * (An addition: nothing that existed changed, so ADAISP_ABI_VERSION stays 9.)
 * src: the decoded images as adaisp_unprocess reads them, packed at any byte offsets; image b is desc[b].h x desc[b].w at
 * src + desc[b].src_offset and stands at (top, left) of an S x S letterbox frame whose other pixels are `fill` (one BGR
 * triple: B in bits 0-7, G in 8-15, R in 16-23). dst: B frames of S x S x 3 bytes, frame b at dst + b * S * S * 3.
 * All arithmetic is integer (64-bit sums wrap modulo 2^64), so the result is defined bit for bit. For output pixel (x, y):
 *     fx = m0 * x + m1 * y + m2,  fy = m3 * x + m4 * y + m5        m[]: the inverse map, Q16
 *     X = fx >> 16, Y = fy >> 16 (arithmetic shift: floor);  ax = (fx >> 11) & 31, ay = (fy >> 11) & 31
 *     P(i, j) = the source pixel at row j - top, column i - left if that lies in [0, h) x [0, w), else fill; each of the
 *               four taps resolved on its own
 *     v = ((32 - ax) (32 - ay) P(X, Y) + ax (32 - ay) P(X + 1, Y) + (32 - ax) ay P(X, Y + 1) + ax ay P(X + 1, Y + 1) + 512)
 *         >> 10, per channel
 * Coordinates are pixel indices with no half-pixel shift (cv2.warpAffine's convention). The identity map (65536, 0, 0, 0,
 * 65536, 0) with lut = -1 reproduces the letterboxed frame exactly.
 * With 0 <= lut < n_luts the warped (b, g, r) then goes through table T = luts + 768 * lut; every `/` divides non-negative
 * integers and rounds down, so (2 n + d) / (2 d) is n / d to nearest, halves up:
 *     V = max(b, g, r), d = V - min(b, g, r);  S = 0 if V = 0, else (255 d + V / 2) / V
 *     H = 0 if d = 0; else n = 30 (g - b) (+ 180 d if negative) when V = r, else 30 (b - r) + 60 d when V = g, else
 *         30 (r - g) + 120 d;  H = (2 n + d) / (2 d), 180 becoming 0        (cv2.COLOR_BGR2HSV's 8-bit H in [0, 180))
 *     H' = T[H] mod 180, S' = T[256 + S], V' = T[512 + V]
 *     i = H' / 30, f = H' - 30 i;  p = (V' (255 - S') + 127) / 255;  q = (V' (7650 - S' f) + 3825) / 7650;
 *     t = (V' (7650 - S' (30 - f)) + 3825) / 7650
 *     (r, g, b) = (V', t, p), (q, V', p), (p, V', t), (p, q, V'), (t, p, V'), (V', p, q) for i = 0 .. 5
 * Any other lut (-1 by convention) leaves the colours as they are. An image whose placement does not fit the frame, or whose
 * pixels do not lie inside src_bytes, comes out all `fill` and is never read from. Every byte of dst is written.
 * ADAISP_EINVAL: null src / desc / dst, null luts with n_luts > 0, n_luts < 0, B < 1, S < 1, fill > 0xFFFFFF;
 * ADAISP_ESHAPE: B > 65535 or S > 32768; all checked before anything touches a device. No allocation, no host
 * synchronisation: capturable in a hipGraph.
 */
typedef struct adaisp_augment_desc {
    int64_t src_offset;        /* byte offset of the image's first pixel in src                                  */
    int32_t h, w, top, left;   /* un-padded size and its placement in the S x S frame (adaisp_unprocess_desc's)  */
    int64_t m[6];              /* Q16 inverse map: output pixel -> frame coordinates                             */
    int32_t lut;               /* index of the image's 768-byte table in luts; -1: no colour change              */
    int32_t reserved;
} adaisp_augment_desc;
int adaisp_augment_u8(const uint8_t* src, size_t src_bytes, const adaisp_augment_desc* desc, const uint8_t* luts,
                      int n_luts, uint8_t* dst, int B, int S, unsigned fill, void* stream);

/*
 * Mosaic and mixup, the other half of the reference's augment=True branch: the same pass as adaisp_augment_u8 over a canvas
 * made of up to four sources (`load_mosaic`, dataloaders.py:758-814) and the blend of two such canvases (`mixup`,
 * augmentations.py:289-294), uint8 HWC BGR -> uint8 HWC BGR, one launch per batch. (An addition: ADAISP_ABI_VERSION stays 9.)
 * src, luts, n_luts, dst, B, S as adaisp_augment_u8's. desc: a DEVICE array of B records. Image b has 1 or 2 layers; a layer
 * is a Q16 inverse map m[6] (output pixel -> canvas coordinates), a `fill` (adaisp_augment_u8's packed BGR triple; bits 24-31
 * ignored) and its first n_tiles tiles (n_tiles taken into [0, 4]); a tile is a source image of h x w pixels at
 * src + src_offset, a half-open rectangle [x0, x1) x [y0, y1) of the canvas and (dx, dy): canvas pixel (i, j) of the rectangle
 * is the source's row j - dy, column i - dx. The canvas has no bounds of its own. For output pixel (x, y) and each layer:
 *     fx, fy, X, Y, ax, ay as adaisp_augment_u8's, from the layer's m[]
 *     P(i, j) = the source pixel of the first tile (in index order) with x0 <= i < x1 and y0 <= j < y1, else the layer's fill;
 *               each of the four taps resolved on its own, nothing clamped: taps that straddle a seam between two tiles, or
 *               between a tile and the fill, blend the two
 *     v = adaisp_augment_u8's ((32 - ax) (32 - ay) P(X, Y) + ... + 512) >> 10, per channel
 * With two layers (the record's n_layers = 2 and the launch's n_layers = 2), v0 and v1 their values and mix taken into
 * [0, 65536]:
 *     v = (mix * v0 + (65536 - mix) * v1) >> 16, per channel         (rounds down, as the reference's .astype(np.uint8))
 * else v = v0 and layer 1 is not looked at. With 0 <= lut < n_luts the table chain of adaisp_augment_u8 follows.
 * A tile is absent, never matched and never read from, when h or w lies outside [0, 32768], x1 < x0 or y1 < y0, its rectangle
 * maps outside its own source (x0 - dx < 0, x1 - dx > w, y0 - dy < 0 or y1 - dy > h), or src_offset < 0 or
 * src_offset + h * w * 3 > src_bytes. Every byte of dst is written.
 * "A single image is one layer with one tile": the record with layer[0] = {m, fill, 1, {src_offset, h, w, left, top, left + w,
 * top + h, left, top}}, n_layers = 1 and the same lut gives the frame adaisp_augment_u8 gives for an image that fits its frame,
 * byte for byte.
 * n_layers (the argument): the largest n_layers of the records, 1 or 2; with 1 every image is made from its layer 0 alone.
 * ADAISP_EINVAL: null src / desc / dst, null luts with n_luts > 0, n_luts < 0, B < 1, S < 1, n_layers outside {1, 2};
 * ADAISP_ESHAPE: B > 65535 or S > 32768; all checked before anything touches a device. The records live on the device, so
 * their n_layers, n_tiles and mix are the caller's to check (adaptiveisp_amd/_lib.py mosaic_u8 does, on the host copy); the
 * kernel takes them into range as said above. No allocation, no host synchronisation: capturable in a hipGraph.
 * Byte layout (little endian, no padding): tile 40 bytes: src_offset at 0, h 8, w 12, x0 16, y0 20, x1 24, y1 28, dx 32, dy 36;
 * layer 216 bytes: m at 0, fill 48, n_tiles 52, tile[t] at 56 + 40 t; record 448 bytes: layer[l] at 216 l, n_layers 432, mix 436,
 * lut 440, reserved 444.
 */
typedef struct adaisp_mosaic_tile {
    int64_t src_offset;        /* byte offset of the source's first pixel in src                                 */
    int32_t h, w;              /* the source's size                                                              */
    int32_t x0, y0, x1, y1;    /* the canvas rectangle it fills, half open                                       */
    int32_t dx, dy;            /* source column = i - dx, source row = j - dy                                    */
} adaisp_mosaic_tile;
typedef struct adaisp_mosaic_layer {
    int64_t m[6];              /* Q16 inverse map: output pixel -> canvas coordinates                            */
    uint32_t fill;             /* the canvas where no tile is: B | G << 8 | R << 16                              */
    int32_t n_tiles;           /* 0 .. 4                                                                         */
    adaisp_mosaic_tile tile[4];
} adaisp_mosaic_layer;
typedef struct adaisp_mosaic_desc {
    adaisp_mosaic_layer layer[2];
    int32_t n_layers;          /* 1, or 2: layer 0 blended over layer 1                                          */
    int32_t mix;               /* Q16 weight of layer 0, 0 .. 65536                                              */
    int32_t lut;               /* index of the image's 768-byte table in luts; -1: no colour change              */
    int32_t reserved;
} adaisp_mosaic_desc;
int adaisp_mosaic_u8(const uint8_t* src, size_t src_bytes, const adaisp_mosaic_desc* desc, const uint8_t* luts, int n_luts,
                     uint8_t* dst, int B, int S, int n_layers, void* stream);

/*
 * Raw-capture loader: real sensor planes -> the letterboxed [B,3,S,S] fp32 batch in one launch (demosaic, per-channel gain,
 * resample, placement). The plane is read once, 2 bytes per native pixel, and only the batch is written: the full-resolution
 * colour image never exists in memory.
 * src: uint16 [src_h, src_w] colour-filter-array planes, row-major, packed at any EVEN byte offsets (src itself 2-byte
 * aligned). desc: a DEVICE array of B records. For image b, with pattern / method / black_level / white_level as
 * adaisp_demosaic_rects_ex:
 *   demosaic   D_c(j, i) = what adaisp_demosaic_rects_ex gives for a rectangle that is the whole plane at origin (0, 0), bit
 *              for bit: CFA phase relative to the plane's first sample, mirrors at the plane's edges, odd sides allowed (the
 *              crop continued by its mirror), nothing clamped
 *   gain       V_c(j, i) = D_c(j, i) * gain[c]                                   (one fp32 multiply)
 *   resample   taps in `tabs` (32-bit words, floats by their bits), CSR in adaisp_resize_u8's AREA layout:
 *              at tab_x: ptr[w + 1], idx[nnz], weight[nnz] (src_w -> w), at tab_y the same over h (src_h -> h); the host builds
 *              them (adaptiveisp_amd/resize.py, raw_table: the area weights when shrinking, two-tap fp32 bilinear when
 *              enlarging, one tap of weight 1 when equal). Horizontal pass, then vertical pass, each a sequence of one fp32
 *              multiply then one fp32 add in tap order, starting from 0.0f (no FMA):
 *                  T_c(j, x):    t = t + wx * V_c(j, idx)      over the taps of x
 *                  out_c(y, x):  acc = acc + wy * T_c(idx, x)  over the taps of y
 *              source indices read from the taps are clamped to the plane
 *   placement  the h x w result at (top, left) of out[b]; every other sample of out[b] is exactly 0
 * out[b] is all zero when the placement does not fit the frame, src_h < 2 or src_w < 2, the plane does not lie inside
 * src_bytes, the taps do not lie inside tab_words, or src_offset is odd. Every byte of out is written by every call.
 * ADAISP_EINVAL: null pointers, an odd src, B < 0, S < 1, unknown pattern or method, white_level <= black_level;
 * ADAISP_ESHAPE: B > 65535 or S > 32768; B == 0 is ok and launches nothing; all checked before anything touches a device.
 * No allocation, no host synchronisation: capturable in a hipGraph.
 */
typedef struct adaisp_raw_desc {
    int64_t src_offset;        /* byte offset of the plane's first sample in src (even)                          */
    int32_t src_h, src_w;      /* native plane size; each >= 2, any parity                                       */
    int32_t h, w, top, left;   /* resampled size and its placement in the S x S frame                            */
    int64_t tab_x, tab_y;      /* word offsets in tabs of the horizontal (src_w -> w) / vertical taps            */
    float   gain[3];           /* R, G, B multipliers applied to the demosaiced values (1 = none)                */
    float   reserved;
} adaisp_raw_desc;
int adaisp_raw_load(const uint8_t* src, size_t src_bytes, const adaisp_raw_desc* desc, const int32_t* tabs,
                    size_t tab_words, float* out, int B, int S, int pattern, int method, float black_level,
                    float white_level, void* stream);

/*
 * Raw-capture correction: what a real sensor needs before the demosaic, in one launch over a batch: defect pixels, lens
 * shading, per-position black levels and scale. Reads the packed uint16 planes in src, writes corrected uint16 planes of the
 * same sizes into dst; adaisp_raw_load / adaisp_demosaic_rects_ex then run on dst with one black level (black_out) and one
 * white level. Everything is keyed by the POSITION k = 2 * (y & 1) + (x & 1) in the 2 x 2 tile (the order of the letters in
 * the colour filter's name, the order in which cameras report black levels and DNG lays out gain maps): the function takes
 * no pattern. desc: a DEVICE array of B records. Per sample (y, x) of image b, in this order, every operation one fp32
 * operation (no FMA); the order and the roundings are part of the interface:
 *   defect   v = the sample; n0..n7 = the samples of the same position at (y +- 2 or y, x +- 2 or x), centre excluded, all read
 *            from src (never corrected values), mirrored without edge repeat at the plane's edges (period 2n - 2: the mirror
 *            keeps the position); hi = max n, lo = min n, as integers.
 *            dpc >= 0 and v > hi + dpc: v = hi; else dpc >= 0 and v + dpc < lo: v = lo.
 *   shading  g = 1.0f when grid < 0; else fy = (float)y * step_y, iy = min((int)fy, grid_h - 2), ty = fy - (float)iy, the
 *            same in x, and with T = gains + grid + k * grid_h * grid_w:
 *                a = T[iy][ix] + tx * (T[iy][ix + 1] - T[iy][ix]),  b the same on row iy + 1,  g = a + ty * (b - a)
 *   levels   u = ((float)v - black[k]) * g, then * scale[k], then + black_out
 *   store    uint16 of rintf(u) (ties to even) clamped to [0, 65535]; NaN gives 0
 * With dpc < 0, grid < 0, black[k] = black_out and scale[k] = 1 the output is a copy of the input.
 * An image is skipped, and no byte of dst written for it, when an offset is odd, negative or out of range, its plane does not
 * lie inside src_bytes / dst_bytes, a side is under 2, grid >= 0 with a grid side under 2 or a table that does not lie inside
 * gain_words, or a scale is not finite.
 * ADAISP_EINVAL: null src / dst / desc, null gains with gain_words > 0, an odd src or dst, B < 0; ADAISP_EALIAS: the byte
 * ranges [src, src + src_bytes) and [dst, dst + dst_bytes) overlap (the defect rule reads neighbours: no in-place);
 * ADAISP_ESHAPE: B > 65535; B == 0 is ok and launches nothing; all checked before anything touches a device.
 * No allocation, no host synchronisation: capturable in a hipGraph.
 */
typedef struct adaisp_rawfix_desc {
    int64_t src_offset;        /* byte offset of the plane's first sample in src (even)                          */
    int64_t dst_offset;        /* byte offset of the corrected plane in dst (even)                               */
    int32_t src_h, src_w;      /* plane size; each >= 2, any parity                                              */
    int64_t grid;              /* word offset in gains of this image's [4][grid_h][grid_w] fp32 table; -1: none  */
    int32_t grid_h, grid_w;    /* each >= 2 when grid >= 0                                                       */
    float   step_y, step_x;    /* (grid_h - 1) / (src_h - 1), (grid_w - 1) / (src_w - 1) in fp32, from the host  */
    float   black[4];          /* black level per position k                                                     */
    float   scale[4];          /* per position: (white_out - black_out) / (white_in - black[k]) in fp32          */
    float   black_out;         /* pedestal of the corrected plane                                                */
    int32_t dpc;               /* defect threshold in input counts; < 0: no defect correction                    */
    int32_t reserved[2];
} adaisp_rawfix_desc;
int adaisp_raw_correct(const uint8_t* src, size_t src_bytes, uint8_t* dst, size_t dst_bytes,
                       const adaisp_rawfix_desc* desc, const float* gains, size_t gain_words, int B, void* stream);

/*
 * Image export: planar fp32 RGB img [B,3,H,W] -> interleaved uint8 BGR out [B,H,W,3] (cv2.imwrite's channel order), in one
 * launch, with the arithmetic of the reference's `save_img` (util.py:21-40) and OpenCV's float -> 8U conversion:
 * NaN -> 0, clip to [0, 1], * 255.0f in fp32, round half to even. Any pointer alignment (16-byte loads where the
 * alignment and H*W % 4 == 0 allow). No allocation, no host synchronisation. B <= 65535.
 */
int adaisp_export_u8(const float* img, uint8_t* out, int B, int H, int W, void* stream);

/*
 * NonLocalMeansGray(search_window_size, patch_size).forward(rgb, h) for ANY odd sizes — isp/denoise.py:93-119 (class default
 * 21 / 7; the ISP's DenoiseFilter constructs 11 / 5, isp/filters.py:577, which ADAISP_OP_NLM serves with the tuned kernel).
 * Luminance 0.299 R + 0.587 G + 0.114 B of the CLIPPED image (rgb_to_luminance :11-17), patch distance = box sum of squared
 * differences under torch.roll's circular wrap, weight exp(-sqrt(relu(D)) / (relu(h) + 1e-8)), colours = the input as given,
 * result clamped to [0, 1]. h: one value per image, `h_stride` floats apart. `workspace` (adaisp_nlm_general_workspace_bytes:
 * one fp32 luminance plane per image) is caller-owned scratch. A plain gather kernel — O(search^2 patch^2) per pixel — for
 * configurations the ISP path does not use. `out` must not overlap `img`.
 */
size_t adaisp_nlm_general_workspace_bytes(int B, int H, int W);
int adaisp_nlm_general(const float* img, float* out, const float* h, int h_stride, void* workspace, size_t workspace_bytes,
                       int B, int H, int W, int search_window_size, int patch_size, void* stream);

/* AdaptiveAvgPool2d((64,64)) of a [B,3,H,W] image: agent.py:85,97, value.py:61,63. */
int adaisp_pool64(const float* img, float* pooled, int B, int H, int W, void* stream);

/*
 * Backward of adaisp_pool64: grad_pooled [B,3,64,64] -> grad_img [B,3,H,W] (every pixel written). The critic sees the
 * retouched image through this pooling (value.py:61-63) and, with cfg.use_TD, the agent loss back-propagates through
 * V(retouch, new_states) into the filter parameters (train.py:281-305): this gradient enters adaisp_backward_params
 * as part of grad_out.
 */
int adaisp_pool64_backward(const float* grad_pooled, float* grad_img, int B, int H, int W, void* stream);

/* ---------------------------------------------------------------------------------------------------------
 * Fused eval path of one policy step (Agent.forward in eval mode, agent.py:88-285; FeatureExtractor
 * agent.py:26-60; Filter.extract_parameters / filter_param_regressor isp/filters.py:65-73 and per class).
 * Weights are the module parameters with BatchNorm folded into the convs (eval statistics), fp32.
 * --------------------------------------------------------------------------------------------------------- */
#define ADAISP_POLICY_MAX_FILTERS 16

enum adaisp_regressor_kind {
    ADAISP_REG_TANH_RANGE     = 0, /* tanh01(x + bias) * scale + lo          (E, CCM, Shr, T, USM, C) */
    ADAISP_REG_EXP_TANH_RANGE = 1, /* exp(tanh01(x + bias) * scale + lo)     (G)                      */
    ADAISP_REG_SIGMOID        = 2, /* 1 / (1 + exp(-x))                      (NLM, S+, BW)            */
    ADAISP_REG_TANH           = 3, /* tanh(x)                                (Ct)                     */
    ADAISP_REG_WB             = 4  /* exp(tanh_range(x*[0,1,1])) / luminance (W), isp/filters.py:258-269 */
};

typedef struct adaisp_regressor {
    int32_t op;      /* kernel op code of the filter (enum adaisp_op)  */
    int32_t n;       /* number of regressed parameters                 */
    int32_t kind;    /* enum adaisp_regressor_kind                     */
    float lo, scale, bias;
} adaisp_regressor;

typedef struct adaisp_policy_finish_args {
    /* inputs */
    const float* hidden;       /* [B][F+1][hid]  LeakyReLU(fc1) of the F filter heads, then the selector's   */
    const float* w_filter;     /* [rows][hid]    fc_filter weights of all heads, stacked in filter order       */
    const float* b_filter;     /* [rows]                                                                        */
    const int32_t* row_filter; /* [rows]         filter index of each stacked row                               */
    const int32_t* row_slot;   /* [rows]         parameter slot of each stacked row inside its filter           */
    const float* w_sel;        /* [F][hid]       selector fc2                                                   */
    const float* b_sel;        /* [F]                                                                           */
    const float* noise;        /* [B][noise_stride]  z; column 0 is the selection noise (agent.py:92)           */
    const float* states;       /* [B][3+F]                                                                      */
    const float* runtime;      /* [F] or NULL (cfg.filter_runtime_penalty off)                                  */
    /* outputs */
    float* params_all;         /* [B][F][param_width] regressed parameters of every filter                      */
    float* packed;             /* [B][param_width]    row of the selected filter (input of adaisp_forward)      */
    int32_t* op_ids;           /* [B]                 op code of the selected filter (-1: all-zero one-hot)     */
    long long* selected;       /* [B]                 selected filter id (int64 like the reference)             */
    float* pdf_out;            /* [B][F]                                                                        */
    float* surrogate;          /* [B]                                                                           */
    float* new_states;         /* [B][3+F]                                                                      */
    float* penalty;            /* [B]                                                                           */
    /* scalars */
    int32_t num_filters, num_rows, hid, param_width, noise_stride;      /* noise_stride >= 1                       */
    int32_t train_mode;        /* 1: pdf_sample, 0: argmax                                                      */
    int32_t forced_id;         /* >= 0: teacher-forced selected_filter_id, < num_filters                        */
    float one_minus_exploration, exploration_over_f;
    float entropy_coef;        /* (1 - progress) * cfg.exploration_penalty                                      */
    float log_num_filters, test_steps, filter_usage_penalty, early_stop_penalty, runtime_lambda;
    adaisp_regressor reg[ADAISP_POLICY_MAX_FILTERS];
} adaisp_policy_finish_args;

/*
 * One folded trunk layer: out = LeakyReLU_0.2(conv2d(in, w, k4 s2 p1) + bias), G independent trunks per launch.
 *   in  [G][B][Cin][Hin][Hin], w [G][Cout][Cin][4][4], bias [G][Cout], out [G][B][Cout][Hin/2][Hin/2].
 * First layer: pass states != NULL; `in` is then the 64x64-pooled image [B,3,Hin,Hin] shared by all trunks and
 * input channels 3..Cin-1 are the per-image constants states[b][c-3] (enrich_image_input, util.py:58-63).
 * Cout must be a multiple of 8.
 */
int adaisp_policy_conv(const float* in, const float* states, int n_state, const float* w, const float* bias,
                       float* out, int G, int B, int Cin, int Hin, int Cout, void* stream);

/* hidden[b][h][j] = LeakyReLU_0.2(b1[h][j] + feats[head_src[h]][b][:] . w1[h][j][:]);  feats [G][B][D], D % 4 == 0 */
int adaisp_policy_fc1(const float* feats, const int32_t* head_src, const float* w1, const float* b1, float* hidden,
                      int B, int D, int NH, int HID, void* stream);

/* Everything after the hidden layers (see struct). `args` is a HOST struct holding DEVICE pointers. */
int adaisp_policy_finish(const adaisp_policy_finish_args* args, int B, void* stream);

/* ---------------------------------------------------------------------------------------------------------
 * Training-mode trunk of the policy / critic networks (FeatureExtractor, agent.py:26-60 / value.py:6-44, in train
 * mode as train.py:258,282-283 runs them): [Conv2d(k4 s2 p1) -> BatchNorm2d(batch statistics) -> LeakyReLU(0.2)] x 4
 * on a 64x64 input, forward and backward, fp32. One call serves G <= 2 trunk INSTANCES:
 *   the agent's two trunks (feature_extractor + action_selection: same input, two parameter sets), or
 *   the critic's two calls of an iteration (V(imgs, states), V(retouch, new_states): two inputs, ONE parameter set —
 *   pass the same `adaisp_trunk_params` twice and share_params = 1: statistics stay per instance, the running
 *   statistics are updated in instance order and the parameter gradients are the sum over instances, in that order).
 * Layer-1 input of instance g: the 3 planes img[g] [B,3,64,64] followed by svec[g] [B,n_state] as constant planes
 * (enrich_image_input, util.py:58-63; for the critic the state vector with its three hand statistics, value.py:65-80).
 * Channels: C[0] = 3 + n_state, C[1..4] the four conv widths (C[1..4] % 16 == 0). Output feat [G][B][C[4]*16] =
 * the last activation flattened channel-major (agent.py:57 reshape). Every reduction (batch statistics, their
 * backward sums, weight gradients) runs in a fixed order: results are bit-reproducible run to run.
 * `workspace` keeps what backward needs (pre-BatchNorm outputs, activations, mean / rstd); `scratch` holds backward
 * temporaries. Sizes: adaisp_trunk_train_workspace_bytes / _scratch_bytes.
 * Layout (private to the library; tests/_trunkref.py restates it to read the stages' buffers): the workspace is G equal
 * blocks, one per instance, each holding for l = 1..4 in turn y_l [B,C[l],H_l,H_l] (H_l = 64 >> l), the activation a_l of
 * the same shape (l < 4 only: a_4 is `feat`), then mean_l and rstd_l, C[l] floats each. The scratch is G equal blocks
 * holding for l = 1..4 dy_l and (l < 4) da_l, shaped like y_l, then B*C[0]*64*64 floats whose head receives the first
 * layer's state-plane gradients [B,n_state,64,64] when dimg is wanted; after the G blocks comes one region for the
 * weight-gradient partial tiles, [chunks*G][C[l]][C[l-1]][16] of the layer that needs the most (0 if none is chunked).
 * --------------------------------------------------------------------------------------------------------- */
#define ADAISP_TRUNK_MAX_G 2
#define ADAISP_TRUNK_LAYERS 4

typedef struct adaisp_trunk_params {
    const float* w[ADAISP_TRUNK_LAYERS];        /* [C[l+1]][C[l]][4][4]                              */
    const float* bias[ADAISP_TRUNK_LAYERS];     /* [C[l+1]]                                          */
    const float* gamma[ADAISP_TRUNK_LAYERS];    /* BatchNorm weight                                  */
    const float* beta[ADAISP_TRUNK_LAYERS];     /* BatchNorm bias                                    */
    float* running_mean[ADAISP_TRUNK_LAYERS];   /* updated in place by the forward (NULL: left alone) */
    float* running_var[ADAISP_TRUNK_LAYERS];
} adaisp_trunk_params;

typedef struct adaisp_trunk_grads {             /* every tensor written (not accumulated into)       */
    float* w[ADAISP_TRUNK_LAYERS];
    float* bias[ADAISP_TRUNK_LAYERS];
    float* gamma[ADAISP_TRUNK_LAYERS];
    float* beta[ADAISP_TRUNK_LAYERS];
} adaisp_trunk_grads;

typedef struct adaisp_trunk_args {
    int32_t G, B, n_state, share_params;
    int32_t C[ADAISP_TRUNK_LAYERS + 1];
    float momentum, eps, slope;                 /* BatchNorm momentum / eps, LeakyReLU slope          */
    const float* img[ADAISP_TRUNK_MAX_G];
    const float* svec[ADAISP_TRUNK_MAX_G];
    adaisp_trunk_params p[ADAISP_TRUNK_MAX_G];
    float* feat;                                /* forward output [G][B][C[4]*16]                     */
    float* workspace;
    size_t workspace_bytes;
    /* backward only */
    const float* dfeat;                         /* [G][B][C[4]*16]                                    */
    adaisp_trunk_grads g[ADAISP_TRUNK_MAX_G];   /* share_params: g[0] only                            */
    float* dimg[ADAISP_TRUNK_MAX_G];            /* [B,3,64,64] or NULL (input gradient not wanted)    */
    float* dsvec[ADAISP_TRUNK_MAX_G];           /* [B,n_state] or NULL (both or neither per instance) */
    float* scratch;
    size_t scratch_bytes;
} adaisp_trunk_args;

size_t adaisp_trunk_train_workspace_bytes(const adaisp_trunk_args* args);
size_t adaisp_trunk_train_scratch_bytes(const adaisp_trunk_args* args);
/* `args` is a HOST struct holding DEVICE pointers. 8 launches. */
int adaisp_trunk_train_fwd(const adaisp_trunk_args* args, void* stream);
/* After adaisp_trunk_train_fwd with the same args / workspace. 11-15 launches. */
int adaisp_trunk_train_bwd(const adaisp_trunk_args* args, void* stream);

/*
 * The critic's hand statistics (value.py:65-80) of G <= 2 batches of 64x64 planes `small` [B,3,64,64]:
 *   svec[b] = [states[b][0..n_state), mean luminance, luminance variance (unbiased, torch.var), mean saturation]
 * i.e. the state vector the critic's trunk reads as constant planes. Backward: dsmall = dsmall_in (or 0) + the gradient
 * of the three statistics given dsvec [B,n_state+3] (torch's rules: clip passes on the closed interval, max / min over
 * channels give the first index on ties, minimum splits a tie); dsmall may alias dsmall_in; instances with
 * dsmall[g] == NULL are skipped. One launch each.
 */
typedef struct adaisp_critic_planes_args {
    int32_t G, B, n_state;
    const float* small[ADAISP_TRUNK_MAX_G];
    const float* states[ADAISP_TRUNK_MAX_G];      /* [B,n_state] (NULL when n_state == 0) */
    float* svec[ADAISP_TRUNK_MAX_G];              /* [B,n_state+3]                        */
    /* backward only */
    const float* dsvec[ADAISP_TRUNK_MAX_G];
    const float* dsmall_in[ADAISP_TRUNK_MAX_G];
    float* dsmall[ADAISP_TRUNK_MAX_G];
} adaisp_critic_planes_args;
int adaisp_critic_planes_fwd(const adaisp_critic_planes_args* args, void* stream);
int adaisp_critic_planes_bwd(const adaisp_critic_planes_args* args, void* stream);

/*
 * Reward / TD target / losses of one RL iteration (train.py:262-305): per-sample vectors of B floats in, the per-sample
 * reward / q_value / advantage and losses = [value_loss, agent_loss] out; backward from dlosses [2] to the five inputs
 * that carry gradients. The same operation order as the element-wise reference arithmetic. One launch each.
 */
typedef struct adaisp_td_args {
    int32_t B, state_dim;                          /* new_states [B,state_dim]: [., stopped, step, usage...] */
    int32_t use_penalty, use_truncated, use_td;
    float detect_loss_weight, all_reward, critic_logit_multiplier, discount_factor, parameter_lr_mul,
          maximum_trajectory_length, max_bri;
    const float *l_in, *l_re, *penalty, *surrogate, *new_states, *old_value, *new_value, *retouch_mean;
    float *reward, *q_value, *advantage, *losses;
    /* backward only */
    const float* dlosses;
    float *d_l_re, *d_penalty, *d_surrogate, *d_old_value, *d_new_value;
} adaisp_td_args;
int adaisp_td_fwd(const adaisp_td_args* args, void* stream);
int adaisp_td_bwd(const adaisp_td_args* args, void* stream);

/*
 * The policy's tail in TRAINING mode (agent.py:103-149, 234-280): from the heads' pre-activations x [B][F][param_width]
 * (fc_filter outputs, zero-padded slots) and the selector's logits [B][F] to everything Agent.forward hands on — the regressed
 * parameter table, pdf, sampled / forced selection, surrogate, packed row + op code for adaisp_forward, state update, penalty —
 * with the arithmetic of adaisp_policy_finish; and its backward: d_x (non-zero on the selected filter's row only: nothing else
 * reaches the pixels) and d_logits from d_packed [B][param_width], d_surrogate [B], d_penalty [B] (any may be NULL = zero).
 * One launch each.
 */
typedef struct adaisp_policy_tail_args {
    int32_t B, num_filters, param_width, noise_stride;
    int32_t sample;            /* 1: pdf_sample with noise[b][0] (training), 0: argmax                 */
    int32_t forced_id;         /* >= 0: teacher-forced selected_filter_id                              */
    float one_minus_exploration, exploration_over_f, entropy_coef, log_num_filters, test_steps, filter_usage_penalty,
          early_stop_penalty, runtime_lambda;
    adaisp_regressor reg[ADAISP_POLICY_MAX_FILTERS];
    const float *x, *logits, *noise, *states, *runtime;       /* runtime [F] or NULL                   */
    float* table;              /* [B][F][param_width] regressed parameters of every filter              */
    float* packed;             /* [B][param_width]                                                      */
    int32_t* op_ids;           /* [B]                                                                   */
    long long* selected;       /* [B]  (read by the backward)                                           */
    float* pdf;                /* [B][F] (read by the backward)                                         */
    float *surrogate, *new_states, *penalty;                  /* [B], [B][3+F], [B]                    */
    /* backward only */
    const float *d_packed, *d_surrogate, *d_penalty;
    float *d_x, *d_logits;
    /* non-NULL: the entropy coefficient is read from this DEVICE float at run time instead of `entropy_coef` (a launch captured
     * in a hipGraph is replayed with the coefficient of its iteration: train.py:258 feeds `progress` anew every iteration) */
    const float* entropy_coef_dev;
} adaisp_policy_tail_args;
int adaisp_policy_tail_fwd(const adaisp_policy_tail_args* args, void* stream);
int adaisp_policy_tail_bwd(const adaisp_policy_tail_args* args, void* stream);

/*
 * stats[b] = (mean, number of non-finite values) of image b of a batch of B images of n floats each — what the TD target's
 * brightness test (train.py:287-291) and the replay guard (train.py:374-381) read, in one pass over the batch. `workspace`:
 * B * 128 floats. Fixed summation order. Two launches.
 */
int adaisp_image_stats(const float* img, float* stats, float* workspace, int B, long n, void* stream);

/*
 * torch.nn.utils.clip_grad_norm_(params, max_norm) followed by torch.optim.Adam.step() (train.py:341-351; amsgrad off, no weight
 * decay) over a table of fp32 tensors in three launches. `table` is a DEVICE array of `ntensors` entries: parameter, gradient,
 * first / second moment (updated in place), the tensor's step count AFTER this step (a device float, as torch's fused Adam keeps
 * it), element count, and `chunk0` = the number of 4096-element chunks of the tensors before it (ascending); `nchunks` their total.
 * `workspace`: nchunks + 2 floats; afterwards workspace[nchunks] = the clip coefficient, workspace[nchunks + 1] = the total norm.
 * max_norm <= 0: no clipping. Fixed summation order; the update arithmetic of torch's fused Adam.
 */
typedef struct adaisp_adam_tensor {
    float* p;
    const float* g;
    float* m;
    float* v;
    const float* step;
    long n, chunk0;
} adaisp_adam_tensor;
int adaisp_clip_adam_step(const adaisp_adam_tensor* table, int ntensors, long nchunks, float* workspace, float max_norm, double lr,
                          double beta1, double beta2, double eps, void* stream);
/* The same with the learning rate read from a DEVICE double at run time (`lr_dev`): the launches of a captured iteration follow
 * the LambdaLR schedule (train.py:206-218, 350-351) without a new kernel argument. Same arithmetic, same three launches. */
int adaisp_clip_adam_step_dev(const adaisp_adam_tensor* table, int ntensors, long nchunks, float* workspace, float max_norm,
                              const double* lr_dev, double beta1, double beta2, double eps, void* stream);

/*
 * The policy's parameter heads in TRAINING mode, forward and backward on the filters' own parameter tensors (agent.py:103-116: per
 * filter `fc1` D -> hid, LeakyReLU 0.2, `fc_filter` hid -> n_f; agent.py:117-121: the selector's `fc1` D -> hid on ITS trunk's features,
 * LeakyReLU, `fc2` hid -> F). Forward (2 launches): hidden [B][F+1][hid] = the pre-activations of every fc1 (group F = the selector),
 * x [B][F][pw] = every fc_filter's output, zero in the slots >= n_f (what adaisp_policy_tail_fwd reads), logits [B][F]. Backward
 * (4 launches) from dx / dlogits: the gradient of every weight and bias into the caller's tensors (written, not accumulated) and of
 * both feature rows; `dhid` [B][F+1][hid] and `part` [(F+1)][B][D] are scratch. Every sum in a fixed order. B <= 8, hid a multiple of
 * 8 and at most 256, D a multiple of 1024.
 */
#define ADAISP_HEADS_MAX_B 8
typedef struct adaisp_heads_args {
    int32_t B, F, D, hid, pw;
    int32_t n[ADAISP_POLICY_MAX_FILTERS];
    const float *feat_f, *feat_s;                              /* [B][D] each                                     */
    const float *w1[ADAISP_POLICY_MAX_FILTERS], *b1[ADAISP_POLICY_MAX_FILTERS];   /* [hid][D], [hid]            */
    const float *wf[ADAISP_POLICY_MAX_FILTERS], *bf[ADAISP_POLICY_MAX_FILTERS];   /* [n_f][hid], [n_f]          */
    const float *ws1, *bs1, *ws2, *bs2;                        /* selector: [hid][D], [hid], [F][hid], [F]       */
    float *hidden, *x, *logits;
    /* backward only */
    const float *dx, *dlogits;
    float *dhid, *part;
    float *dw1[ADAISP_POLICY_MAX_FILTERS], *db1[ADAISP_POLICY_MAX_FILTERS], *dwf[ADAISP_POLICY_MAX_FILTERS], *dbf[ADAISP_POLICY_MAX_FILTERS];
    float *dws1, *dbs1, *dws2, *dbs2, *dfeat_f, *dfeat_s;
} adaisp_heads_args;
int adaisp_heads_fwd(const adaisp_heads_args* args, void* stream);
int adaisp_heads_bwd(const adaisp_heads_args* args, void* stream);

/* Number of regressed parameters an op reads per image (0 for ADAISP_OP_ZERO, -1 if unknown). */
int adaisp_num_params(int op);

const char* adaisp_strerror(int code);
int adaisp_abi_version(void);

#ifdef __cplusplus
}
#endif
#endif /* ADAISP_H_ */
