"""Float64 numpy restatement of the simulated Bayer sensor (what adaisp_unprocess_bayer computes in fp32): the colour
filter sampling of tests/_unprocessref.unprocess_clean (the reference's `unprocess` ends in `mosaic`,
isp/unprocess_np.py:217-245, :82-98; `reconstruct_bayer` :111-128 lays the four planes out), the quantiser, and the
rectangle demosaic of adaisp_demosaic_rects built on the C oracle's whole-frame demosaic. Pinned to
tests/golden/bayer.npz by tests/test_bayer_host.py and used by the GPU tests at any shape."""
import numpy as np

import _unprocessref as U

CFA = {"RGGB": 0, "GRBG": 1, "GBRG": 2, "BGGR": 3}      # 2 * ry + rx: where the red sample sits in the 2 x 2 cell


def cfa_channels(h, w, pattern):
    """[h, w] int: the channel (0 R, 1 G, 2 B) pixel (iy, ix) of an image keeps under `pattern` (a name or 0..3)."""
    pat = CFA[pattern.upper()] if isinstance(pattern, str) else int(pattern)
    py = (np.arange(h)[:, None] - (pat >> 1)) & 1
    px = (np.arange(w)[None, :] - (pat & 1)) & 1
    return np.where(py == px, 2 * py, 1)


def mosaic_plane(img_hwc, pattern="RGGB"):
    """The [h, w] colour-filter-array plane of an HWC RGB image: every pixel keeps its CFA channel."""
    h, w = img_hwc.shape[:2]
    return np.take_along_axis(img_hwc, cfa_channels(h, w, pattern)[..., None], axis=-1)[..., 0]


def quantise(v, black, white):
    """clamp(rint(v * (white - black)) + black, 0, 65535) as uint16, in v's own precision (rint: half to even)."""
    v = np.asarray(v)
    t = v.dtype.type
    return np.clip(np.rint(v * t(white - black)) + t(black), 0, 65535).astype(np.uint16)


def sensor_plane(bgr_u8, rgb2cam, rgb_gain, red_gain, blue_gain, pattern="RGGB", prescale=1.0, ratio=1.0):
    """uint8 HWC BGR -> the float64 [h, w] plane `reconstruct_bayer(unprocess(rgb)[0], pattern)` holds (noise-free)."""
    return mosaic_plane(U.unprocess_clean(bgr_u8, rgb2cam, rgb_gain, red_gain, blue_gain, prescale, ratio), pattern)


def demosaic_rect(plane, h, w, top, left, pattern=0, black=0.0, white=65535.0):
    """adaisp_demosaic_rects of one uint16 [S, S] plane on the C oracle: the whole-frame demosaic of the crop (an odd side
    continued by one mirrored row / column, row h = row h - 2, which is dropped again), zeros around it -> fp32 [3, S, S].
    An image with a side under 2, or a placement that does not fit, gives zeros."""
    import oracle
    S = plane.shape[-1]
    out = np.zeros((3, S, S), np.float32)
    if h < 2 or w < 2 or top < 0 or left < 0 or top + h > S or left + w > S:
        return out
    crop = np.ascontiguousarray(plane[top:top + h, left:left + w])
    if h & 1:
        crop = np.concatenate([crop, crop[h - 2:h - 1]], axis=0)
    if w & 1:
        crop = np.concatenate([crop, crop[:, w - 2:w - 1]], axis=1)
    pat = CFA[pattern.upper()] if isinstance(pattern, str) else int(pattern)
    out[:, top:top + h, left:left + w] = oracle.demosaic(crop[None], pat, black, white)[0][:, :h, :w]
    return out
