// Per-pixel math of the two demosaics (include/adaisp.h: adaisp_demosaic*, adaisp_raw_load), written once for the
// whole-frame / rectangle kernels of isp_demosaic.hip and the fused loader of isp_raw_load.hip: the border reflection
// and, given a site's neighbourhood, its three colours. How the neighbourhood reaches a lane (LDS tile, register window,
// global memory) is the kernel's own business; the expressions here fix the rounding, so every kernel that calls them
// gives the same bits.
#pragma once
#include <hip/hip_runtime.h>

namespace adaisp {

// one reflection is all a valid output of the 3 x 3 filter ever needs; the clamp only keeps the staging of rows / columns
// beyond the image (tiles that overhang it) inside the allocation
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
__device__ __forceinline__ void mhc_site_sums(float c, float a1h, float a1v, float a2h, float a2v, float d, int py, int px,
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

}  // namespace adaisp
