"""numpy int64 restatement of adaisp_augment_u8, written from the header comment of csrc/isp_augment.hip (and
include/adaisp.h): the fixed-point affine warp of a letterboxed uint8 BGR image and the integer BGR -> HSV -> tables ->
BGR chain. It calls no package code. Every division below is `//` on non-negative int64 values."""
import numpy as np

IDENTITY = (65536, 0, 0, 0, 65536, 0)


def fill_triple(fill):
    """The packed fill (B | G << 8 | R << 16) as a (b, g, r) tuple."""
    return (fill & 255, (fill >> 8) & 255, (fill >> 16) & 255)


def letterboxed(img, S, top, left, fill=0):
    """The S x S x 3 frame the warp samples: `img` at (top, left), `fill` around it."""
    out = np.empty((S, S, 3), np.uint8)
    out[...] = fill_triple(fill)
    h, w = img.shape[:2]
    out[top:top + h, left:left + w] = img
    return out


def warp(img, top, left, m, S, fill=0):
    """uint8 [h,w,3] at (top, left) of the S x S frame, through the Q16 inverse map m[0..5] -> uint8 [S,S,3]."""
    h, w = img.shape[:2]
    fits = top >= 0 and left >= 0 and top <= S - h and left <= S - w
    m = [np.int64(v) for v in m]
    x = np.arange(S, dtype=np.int64)[None, :]
    y = np.arange(S, dtype=np.int64)[:, None]
    with np.errstate(over="ignore"):
        fx = m[0] * x + m[1] * y + m[2]
        fy = m[3] * x + m[4] * y + m[5]
    X, Y = fx >> 16, fy >> 16
    ax, ay = (fx >> 11) & 31, (fy >> 11) & 31
    pad = np.array(fill_triple(fill), np.int64)
    flat = img.reshape(-1, 3).astype(np.int64) if img.size else np.zeros((1, 3), np.int64)

    def P(i, j):
        ix, iy = i - left, j - top
        inside = (ix >= 0) & (ix < w) & (iy >= 0) & (iy < h) & bool(fits)
        k = np.where(inside, iy * w + ix, 0)
        return np.where(inside[..., None], flat[k], pad)

    ax, ay = ax[..., None], ay[..., None]
    v = ((32 - ax) * (32 - ay) * P(X, Y) + ax * (32 - ay) * P(X + 1, Y) + (32 - ax) * ay * P(X, Y + 1)
         + ax * ay * P(X + 1, Y + 1) + 512) >> 10
    return v.astype(np.uint8)


def bgr2hsv(bgr):
    """[...,3] (b, g, r) in [0, 255] -> (H in [0, 180), S, V) int64 arrays."""
    c = np.asarray(bgr).astype(np.int64)
    b, g, r = c[..., 0], c[..., 1], c[..., 2]
    V = np.maximum(np.maximum(b, g), r)
    d = V - np.minimum(np.minimum(b, g), r)
    S = np.where(V > 0, (255 * d + V // 2) // np.maximum(V, 1), 0)
    nr = 30 * (g - b)
    nr = np.where(nr < 0, nr + 180 * d, nr)
    n = np.where(V == r, nr, np.where(V == g, 30 * (b - r) + 60 * d, 30 * (r - g) + 120 * d))
    H = np.where(d > 0, (2 * n + d) // np.maximum(2 * d, 1), 0)
    H = np.where(H >= 180, H - 180, H)
    return H, S, V


def hsv2bgr(H, S, V):
    """(H, S, V) int arrays (H taken mod 180) -> [...,3] (b, g, r) int64."""
    H, S, V = (np.asarray(a).astype(np.int64) for a in (H, S, V))
    H = H % 180
    i = H // 30
    f = H - 30 * i
    p = (V * (255 - S) + 127) // 255
    q = (V * (7650 - S * f) + 3825) // 7650
    t = (V * (7650 - S * (30 - f)) + 3825) // 7650
    r = np.choose(i, [V, q, p, p, t, V])
    g = np.choose(i, [t, V, V, q, p, p])
    b = np.choose(i, [p, p, t, V, V, q])
    return np.stack([b, g, r], axis=-1)


def colour(bgr, lut):
    """uint8 [...,3] through one image's 768-byte table (hue, saturation, value) -> uint8 [...,3]."""
    T = np.asarray(lut, np.uint8).reshape(768).astype(np.int64)
    H, S, V = bgr2hsv(bgr)
    return hsv2bgr(T[H], T[256 + S], T[512 + V]).astype(np.uint8)


def augment(img, top, left, m, S, fill=0, lut=None):
    """One image of adaisp_augment_u8: warp, then the colour tables when `lut` is given."""
    out = warp(img, top, left, m, S, fill)
    return out if lut is None else colour(out, lut)
