"""Float64 numpy restatement of the gradient-corrected demosaic (Malvar, He, Cutler 2004) that adaisp_demosaic_ex /
adaisp_demosaic_rects_ex compute with ADAISP_DEMOSAIC_MHC (include/adaisp.h states the filters): the 5 x 5 sums on the
un-normalised samples raw - black, continued over the border by np.pad(mode="reflect"), then the kernel's two fp32
multiplies. The sums are exact in either precision (asserted), so the restatement defines the output bit for bit.
Used by tests/test_mhc_host.py (properties of the restatement itself) and tests/test_gpu_mhc.py (the kernels)."""
import numpy as np

CFA = {"RGGB": 0, "GRBG": 1, "GBRG": 2, "BGGR": 3}      # 2 * ry + rx: where the red sample sits in the 2 x 2 cell


def _pat(pattern):
    return CFA[pattern.upper()] if isinstance(pattern, str) else int(pattern)


def acc(plane, pattern=0, black=0.0):
    """float64 [3, h, w]: the table's `acc` (8 x the un-normalised colour) at every pixel of a [h, w] plane, h, w >= 2."""
    h, w = plane.shape
    assert h >= 2 and w >= 2
    t = np.pad(np.asarray(plane, np.float64) - float(black), 2, mode="reflect")

    def at(dy, dx):
        return t[2 + dy:2 + dy + h, 2 + dx:2 + dx + w]

    c = at(0, 0)
    a1h, a1v = at(0, -1) + at(0, 1), at(-1, 0) + at(1, 0)
    a2h, a2v = at(0, -2) + at(0, 2), at(-2, 0) + at(2, 0)
    d = at(-1, -1) + at(-1, 1) + at(1, -1) + at(1, 1)
    own = 8 * c
    cross = 4 * c + 2 * (a1h + a1v) - (a2h + a2v)
    diag = 6 * c + 2 * d - 1.5 * (a2h + a2v)
    horiz = 5 * c + 4 * a1h - d - a2h + 0.5 * a2v
    vert = 5 * c + 4 * a1v - d - a2v + 0.5 * a2h
    pat = _pat(pattern)
    py = ((np.arange(h)[:, None] - (pat >> 1)) & 1) * np.ones((1, w), int)   # 0, 0: red site; 1, 1: blue site
    px = ((np.arange(w)[None, :] - (pat & 1)) & 1) * np.ones((h, 1), int)
    red, blue, grow = (py == 0) & (px == 0), (py == 1) & (px == 1), py == 0
    r = np.where(red, own, np.where(blue, diag, np.where(grow, horiz, vert)))      # green site in a red row: red lies W / E
    g = np.where(red | blue, cross, own)
    b = np.where(blue, own, np.where(red, diag, np.where(grow, vert, horiz)))
    return np.stack([r, g, b])


def mhc(plane_u16, pattern=0, black=0.0, white=65535.0):
    """fp32 [3, h, w]: (acc * 0.125f) * (1.0f / (white - black)) for a uint16 [h, w] plane, any h, w >= 2."""
    a = acc(plane_u16, pattern, black)
    assert np.array_equal(2 * a, np.rint(2 * a)) and np.abs(2 * a).max() < 2 ** 24      # exact in fp32 in any order
    inv = np.float32(1) / (np.float32(white) - np.float32(black))
    return a.astype(np.float32) * np.float32(0.125) * inv


def mhc_rect(plane, h, w, top, left, pattern=0, black=0.0, white=65535.0):
    """adaisp_demosaic_rects_ex (MHC) of one uint16 [S, S] plane: `mhc` of the crop, zeros around it -> fp32 [3, S, S].
    An image with a side under 2, or a placement that does not fit, gives zeros."""
    S = plane.shape[-1]
    out = np.zeros((3, S, S), np.float32)
    if h < 2 or w < 2 or top < 0 or left < 0 or top + h > S or left + w > S:
        return out
    out[:, top:top + h, left:left + w] = mhc(plane[top:top + h, left:left + w], pattern, black, white)
    return out
