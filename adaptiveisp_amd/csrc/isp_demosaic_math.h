// Per-pixel math of the two demosaics (include/adaisp.h: adaisp_demosaic*, adaisp_raw_load), written once for the
// whole-frame / rectangle kernel of isp_demosaic.hip and the fused loader of isp_raw_load.hip: the border reflection,
// the conversion of a raw sample and, given a site's neighbourhood, its three colours. How the neighbourhood reaches a
// lane (LDS tile, register window, global memory) is the kernel's own business: it hands raw_site() a function
// at(dy, dx). The expressions here fix the rounding, so every kernel that calls them gives the same bits.
#pragma once
#include <hip/hip_runtime.h>
#include "../../include/adaisp.h"

namespace adaisp {

// one reflection is all a valid output of the 3 x 3 filter ever needs (-1 <= i <= n); the clamp only keeps the staging of
// rows / columns beyond the image (tiles that overhang it) inside the allocation. Cheaper than reflect2(), and the
// bilinear kernel's time shows it.
__device__ __forceinline__ int mirror(int i, int n) {
    const int m = i < 0 ? -i : (i >= n ? 2 * n - 2 - i : i);
    return min(max(m, 0), n - 1);
}

// np.pad(mode="reflect"), period 2n - 2, for every index a valid output reads: -2 <= i <= n + 1 with n >= 2. Two folds:
// on a 2-pixel side -2 -> 2 -> 0 and 3 -> -1 -> 1; n >= 3 needs one. The clamp is for rows / columns further out, which
// only the parts of a tile that overhang the image (or the rectangle) stage and nothing reads. Equal to mirror() on
// -1 <= i <= n.
__device__ __forceinline__ int fold(int i, int n) { return i < 0 ? -i : (i >= n ? 2 * n - 2 - i : i); }
__device__ __forceinline__ int reflect2(int i, int n) { return min(max(fold(fold(i, n), n), 0), n - 1); }

// Bilinear: the NORMALISED samples s = (raw - black) * inv_range of the 3 x 3 neighbourhood; (py, px) the site's phase,
// 0,0 = red site; 1,1 = blue site.
__device__ __forceinline__ void bilinear_site(float c, float n, float so, float w, float e, float nw, float ne, float sw,
                                              float se, int py, int px, float& r, float& g, float& b) {
    const float cross = ((n + so) + (w + e)) * 0.25f;
    const float diag = ((nw + ne) + (sw + se)) * 0.25f;
    const float horiz = (w + e) * 0.5f, vert = (n + so) * 0.5f;
    if (py == 0 && px == 0) { r = c; g = cross; b = diag; }
    else if (py == 0) { r = horiz; g = c; b = vert; }
    else if (px == 0) { r = vert; g = c; b = horiz; }
    else { r = diag; g = cross; b = c; }
}

// Malvar-He-Cutler: the UN-normalised samples t = float(raw) - black; c the centre, a1h = W + E, a1v = N + S,
// a2h = W2 + E2, a2v = N2 + S2, d = NW + NE + SW + SE (all exact for whole-number levels, see isp_demosaic.hip).
__device__ __forceinline__ void mhc_sums(float c, float a1h, float a1v, float a2h, float a2v, float d, int py, int px,
                                         float inv_range, float& r, float& g, float& b) {
    float ar, ag, ab;
    if (py == px) {                                                              // red or blue site
        const float own = 8.0f * c;
        ag = 4.0f * c + 2.0f * (a1h + a1v) - (a2h + a2v);
        const float opp = 6.0f * c + 2.0f * d - 1.5f * (a2h + a2v);
        ar = py == 0 ? own : opp;
        ab = py == 0 ? opp : own;
    } else {                                                                     // green site
        const float horiz = 5.0f * c + 4.0f * a1h - d - a2h + 0.5f * a2v;
        const float vert = 5.0f * c + 4.0f * a1v - d - a2v + 0.5f * a2h;
        ag = 8.0f * c;
        ar = py == 0 ? horiz : vert;                                             // red row: red lies W / E
        ab = py == 0 ? vert : horiz;
    }
    r = (ar * 0.125f) * inv_range;
    g = (ag * 0.125f) * inv_range;
    b = (ab * 0.125f) * inv_range;
}

// A raw sample as the method's filter takes it: bilinear the NORMALISED s = (raw - black) * inv_range, MHC the
// UN-normalised t = float(raw) - black.
template <int METHOD>
__device__ __forceinline__ float raw_sample(unsigned v, float black, float inv_range) {
    const float t = (float)v - black;
    return METHOD == ADAISP_DEMOSAIC_MHC ? t : t * inv_range;
}

// the three colours of a site of phase (py, px) from its neighbourhood at(dy, dx), samples as raw_sample<METHOD> gives
// them: |dy|, |dx| <= 1 for bilinear, <= 2 for MHC
template <int METHOD, class At>
__device__ __forceinline__ void raw_site(At at, int py, int px, float inv_range, float& r, float& g, float& b) {
    const float c = at(0, 0);
    if (METHOD == ADAISP_DEMOSAIC_MHC) {
        const float a1h = at(0, -1) + at(0, 1), a1v = at(-1, 0) + at(1, 0);
        const float a2h = at(0, -2) + at(0, 2), a2v = at(-2, 0) + at(2, 0);
        const float d = (at(-1, -1) + at(-1, 1)) + (at(1, -1) + at(1, 1));
        mhc_sums(c, a1h, a1v, a2h, a2v, d, py, px, inv_range, r, g, b);
    } else {
        bilinear_site(c, at(-1, 0), at(1, 0), at(0, -1), at(0, 1), at(-1, -1), at(-1, 1), at(1, -1), at(1, 1), py, px, r, g,
                      b);
    }
}

}  // namespace adaisp
