"""Training augmentation of the replay loaders (the reference's `augment=True` branch, dataset.py:483-514): the host half.

The random draws, the matrix and the label arithmetic are the reference's (`random_perspective`, `augment_hsv`,
`box_candidates`, `xyxy2xywhn`, the two flips), in its order; the pixels are the device's: adaisp_augment_u8
(csrc/isp_augment.hip) warps the letterboxed 8-bit frame through the Q16 inverse of the drawn matrix, with the flips
folded in, and applies the three HSV tables, all in integer arithmetic. The warp is affine: a non-zero `perspective`
is refused.

Mosaic and mixup (`load_mosaic`, dataloaders.py:758-814; `mixup`, augmentations.py:289-294) are loader arguments
(ImageFolderSource(mosaic=, mixup=)), not Hyp keys: `draw_mosaic`, `mosaic_tiles`, `mosaic_boxes` and `mix_q16` are their
host half, adaisp_mosaic_u8 samples the four-tile canvas (and blends two of them) without ever building it. Copy-paste is not
built: it needs segment polygons, which the loaders do not read, and is a no-op for a dataset without segments."""
import math
import os
import warnings
from typing import NamedTuple

import numpy as np

# the keys this module reads, with the values of the reference's low-augmentation hyper-parameter file
DEFAULTS = dict(hsv_h=0.015, hsv_s=0.7, hsv_v=0.4, degrees=0.0, translate=0.1, scale=0.5, shear=0.0, perspective=0.0,
                flipud=0.0, fliplr=0.5)
NOT_BUILT = ("mosaic", "mixup", "copy_paste")


class Hyp:
    """The augmentation hyper-parameters, under the reference's key names (DEFAULTS). `source`: None (the defaults), a
    dict, a YAML file of the reference's (keys this module does not use are ignored) or another Hyp."""

    def __init__(self, source=None, **over):
        if isinstance(source, Hyp):
            source = source.as_dict()
        elif isinstance(source, (str, os.PathLike)):
            import yaml
            with open(source, errors="ignore") as f:
                loaded = yaml.safe_load(f)
            if not isinstance(loaded, dict):
                raise ValueError(f"{source}: not a mapping of hyper-parameters")
            source = loaded
        elif source is not None and not isinstance(source, dict):
            raise TypeError(f"Hyp takes None, a dict, a YAML path or a Hyp, got {type(source).__name__}")
        given = dict(source or {}, **over)
        for k, default in DEFAULTS.items():
            v = float(given.get(k, default))
            if not math.isfinite(v):
                raise ValueError(f"{k} must be finite, got {given[k]!r}")
            setattr(self, k, v)
        if self.perspective != 0:
            raise ValueError(f"perspective = {self.perspective:g}: the warp kernel is affine (perspective must be 0)")
        for k in ("hsv_h", "hsv_s", "hsv_v", "degrees", "translate", "scale", "shear", "flipud", "fliplr"):
            if getattr(self, k) < 0:
                raise ValueError(f"{k} must be >= 0, got {getattr(self, k):g}")
        if self.scale >= 1:
            raise ValueError(f"scale must be below 1 (the image scale is drawn from [1 - scale, 1 + scale]), got {self.scale:g}")
        ignored = [k for k in NOT_BUILT if given.get(k)]
        if ignored:
            warnings.warn(f"{', '.join(ignored)}: not built (single-image augmentation only); ignored", RuntimeWarning,
                          stacklevel=2)

    def as_dict(self):
        return {k: getattr(self, k) for k in DEFAULTS}

    def describe(self):
        return " ".join(f"{k}={getattr(self, k):g}" for k in DEFAULTS if getattr(self, k) != 0)

    def __eq__(self, other):
        return isinstance(other, Hyp) and self.as_dict() == other.as_dict()

    def __repr__(self):
        return f"Hyp({self.as_dict()})"


class Draw(NamedTuple):
    """One image's augmentation: the forward matrix M = T S R P C (float64 [3,3], frame pixel -> warped pixel, before the
    flips), the drawn scale s, the flips, and the hue / saturation / value tables (uint8 [3,256]) or None."""
    M: np.ndarray
    s: float
    flipud: bool
    fliplr: bool
    luts: np.ndarray


def _perspective(hyp, rng, S, canvas):
    """random_perspective's eight `rng.uniform` and its M = T S R P C for a `canvas` x `canvas` input cropped to S x S
    (canvas = S: border 0; canvas = 2 S: the mosaic's border of -S / 2). Returns (M, s)."""
    C = np.eye(3)
    C[0, 2] = -canvas / 2
    C[1, 2] = -canvas / 2
    P = np.eye(3)
    P[2, 0] = rng.uniform(-hyp.perspective, hyp.perspective)
    P[2, 1] = rng.uniform(-hyp.perspective, hyp.perspective)
    a = rng.uniform(-hyp.degrees, hyp.degrees)
    s = rng.uniform(1 - hyp.scale, 1 + hyp.scale)
    # cv2.getRotationMatrix2D(angle=a, center=(0, 0), scale=s): [[alpha, beta, 0], [-beta, alpha, 0]]
    alpha, beta = s * math.cos(a * math.pi / 180), s * math.sin(a * math.pi / 180)
    R = np.eye(3)
    R[0, 0], R[0, 1], R[1, 0], R[1, 1] = alpha, beta, -beta, alpha
    Sh = np.eye(3)
    Sh[0, 1] = math.tan(rng.uniform(-hyp.shear, hyp.shear) * math.pi / 180)
    Sh[1, 0] = math.tan(rng.uniform(-hyp.shear, hyp.shear) * math.pi / 180)
    T = np.eye(3)
    T[0, 2] = rng.uniform(0.5 - hyp.translate, 0.5 + hyp.translate) * S
    T[1, 2] = rng.uniform(0.5 - hyp.translate, 0.5 + hyp.translate) * S
    return T @ Sh @ R @ P @ C, s


def draw_colour_flips(hyp, rng, nprs):
    """The draws behind the warp, in the reference's order: augment_hsv's one `nprs.uniform(-1, 1, 3)` (not made when all
    three gains are 0: no tables then), the two `rng.random()` of the flips. Returns (luts or None, flipud, fliplr)."""
    luts = None
    if hyp.hsv_h or hyp.hsv_s or hyp.hsv_v:
        r = nprs.uniform(-1, 1, 3) * [hyp.hsv_h, hyp.hsv_s, hyp.hsv_v] + 1
        x = np.arange(0, 256, dtype=r.dtype)
        luts = np.stack([((x * r[0]) % 180).astype(np.uint8), np.clip(x * r[1], 0, 255).astype(np.uint8),
                         np.clip(x * r[2], 0, 255).astype(np.uint8)])
    flipud = rng.random() < hyp.flipud
    fliplr = rng.random() < hyp.fliplr
    return luts, flipud, fliplr


def draw(hyp, rng, nprs, S):
    """The draws of one S x S image, in the reference's order: random_perspective's eight `rng.uniform` (the two
    perspective ones are made at 0 too), augment_hsv's one `nprs.uniform(-1, 1, 3)` (not made when all three gains are 0:
    no tables then), the two `rng.random()` of the flips. `rng`: a random.Random, `nprs`: a np.random.RandomState."""
    M, s = _perspective(hyp, rng, S, S)
    luts, flipud, fliplr = draw_colour_flips(hyp, rng, nprs)
    return Draw(M, s, flipud, fliplr, luts)


def fixed_inverse(M, flipud, fliplr, S):
    """The six Q16 entries adaisp_augment_u8 takes: rint(65536 * inv(F M)), int64, where F mirrors the warped frame
    (x -> S - 1 - x for fliplr, y -> S - 1 - y for flipud): output pixel -> letterbox-frame coordinates."""
    F = np.eye(3)
    if fliplr:
        F[0, 0], F[0, 2] = -1.0, S - 1.0
    if flipud:
        F[1, 1], F[1, 2] = -1.0, S - 1.0
    inv = np.linalg.inv(F @ np.asarray(M, np.float64))
    return np.rint(65536.0 * inv[:2].reshape(-1)).astype(np.int64)


def warp_labels(labels, M, s, flipud, fliplr, S):
    """The loader's label rows [k,5] (class, x, y, w, h normalised to the S x S frame) after the augmentation, float64:
    to pixel xyxy; the four corners through M, their min / max, clipped to the frame (random_perspective,
    augmentations.py:217-235); the rows `box_candidates` keeps (:297-302 against the boxes before the warp times s: over
    2 px a side, area ratio over 0.10, aspect under 100); back to normalised xywh with the clip of
    xyxy2xywhn(clip=True, eps=1e-3); then the flips (y -> 1 - y, x -> 1 - x; dataset.py:505-514)."""
    lb = np.array(labels, np.float64).reshape(-1, 5)
    n = len(lb)
    if not n:
        return lb
    box = np.empty((n, 4))
    box[:, 0] = S * (lb[:, 1] - lb[:, 3] / 2)
    box[:, 1] = S * (lb[:, 2] - lb[:, 4] / 2)
    box[:, 2] = S * (lb[:, 1] + lb[:, 3] / 2)
    box[:, 3] = S * (lb[:, 2] + lb[:, 4] / 2)
    return finish_labels(warp_boxes(np.concatenate([lb[:, :1], box], 1), M, s, S), S, flipud, fliplr)


def warp_boxes(rows, M, s, S):
    """Rows [k,5] of class + pixel xyxy through M (random_perspective, augmentations.py:217-235): the four corners, their
    min / max, clipped to the S x S frame; the rows `box_candidates` keeps (:297-302 against the boxes before the warp times
    s: over 2 px a side, area ratio over 0.10, aspect under 100). Returns class + warped xyxy, float64."""
    rows = np.array(rows, np.float64).reshape(-1, 5)
    n = len(rows)
    if not n:
        return rows
    box = rows[:, 1:]
    xy = np.ones((n * 4, 3))
    xy[:, :2] = box[:, [0, 1, 2, 3, 0, 3, 2, 1]].reshape(n * 4, 2)           # x1y1, x2y2, x1y2, x2y1
    xy = (xy @ np.asarray(M, np.float64).T)[:, :2].reshape(n, 8)
    x, y = xy[:, [0, 2, 4, 6]], xy[:, [1, 3, 5, 7]]
    new = np.stack((x.min(1), y.min(1), x.max(1), y.max(1)), axis=1)
    new[:, [0, 2]] = new[:, [0, 2]].clip(0, S)
    new[:, [1, 3]] = new[:, [1, 3]].clip(0, S)
    eps = 1e-16
    before = box * s
    w1, h1 = before[:, 2] - before[:, 0], before[:, 3] - before[:, 1]
    w2, h2 = new[:, 2] - new[:, 0], new[:, 3] - new[:, 1]
    ar = np.maximum(w2 / (h2 + eps), h2 / (w2 + eps))
    keep = (w2 > 2) & (h2 > 2) & (w2 * h2 / (w1 * h1 + eps) > 0.10) & (ar < 100)
    return np.concatenate([rows[keep, :1], new[keep]], 1)


def finish_labels(rows, S, flipud, fliplr):
    """Rows [k,5] of class + pixel xyxy in the S x S frame -> class + normalised xywh with the clip of
    xyxy2xywhn(clip=True, eps=1e-3), then the flips (y -> 1 - y, x -> 1 - x; dataset.py:505-514)."""
    rows = np.array(rows, np.float64).reshape(-1, 5)
    lb, new = rows.copy(), rows[:, 1:].clip(0, S - 1e-3)
    lb[:, 1] = (new[:, 0] + new[:, 2]) / 2 / S
    lb[:, 2] = (new[:, 1] + new[:, 3]) / 2 / S
    lb[:, 3] = (new[:, 2] - new[:, 0]) / S
    lb[:, 4] = (new[:, 3] - new[:, 1]) / S
    if flipud:
        lb[:, 2] = 1 - lb[:, 2]
    if fliplr:
        lb[:, 1] = 1 - lb[:, 1]
    return lb


# ------------------------------------------------------------------------------------------------- mosaic and mixup
class MosaicDraw(NamedTuple):
    """One four-image mosaic: the dataset indices in placement order (top left, top right, bottom left, bottom right), the
    centre (xc, yc) on the 2S x 2S canvas, the forward matrix M (canvas pixel -> S x S output pixel, before the flips)
    and the drawn scale s."""
    indices: tuple
    centre: tuple
    M: np.ndarray
    s: float


def draw_mosaic(hyp, rng, nprs, S, n, index):
    """load_mosaic's draws for image `index` of a dataset of n, from `rng` in the reference's order (dataloaders.py:762-764,
    804-812): yc then xc, each int(uniform(S / 2, 3 S / 2)); choices(range(n), k=3); the shuffle of the four indices;
    random_perspective's eight uniforms with border (-S / 2, -S / 2): C translates by -S, T uses width = height = S.
    `nprs` is not drawn from (the mixup ratio and the HSV gains are the caller's draws)."""
    yc, xc = (int(rng.uniform(S / 2, 2 * S - S / 2)) for _ in range(2))
    indices = [index] + rng.choices(range(n), k=3)
    rng.shuffle(indices)
    M, s = _perspective(hyp, rng, S, 2 * S)
    return MosaicDraw(tuple(indices), (xc, yc), M, s)


def mosaic_tiles(sizes, centre, S):
    """The four tiles of a mosaic as adaisp_mosaic_u8 takes them: for the (h, w) of the images in placement order and the
    centre (xc, yc), rows (x0, y0, x1, y1, dx, dy), int64 [4,6]: the canvas rectangle `x1a, y1a, x2a, y2a` of
    dataloaders.py:770-783 and (dx, dy) = (padw, padh) = (x1a - x1b, y1a - y1b) of :785-786."""
    xc, yc = centre
    out = np.zeros((4, 6), np.int64)
    for i, (h, w) in enumerate(sizes):
        if i == 0:                                # top left
            x1a, y1a, x2a, y2a = max(xc - w, 0), max(yc - h, 0), xc, yc
            x1b, y1b = w - (x2a - x1a), h - (y2a - y1a)
        elif i == 1:                              # top right
            x1a, y1a, x2a, y2a = xc, max(yc - h, 0), min(xc + w, S * 2), yc
            x1b, y1b = 0, h - (y2a - y1a)
        elif i == 2:                              # bottom left
            x1a, y1a, x2a, y2a = max(xc - w, 0), yc, xc, min(S * 2, yc + h)
            x1b, y1b = w - (x2a - x1a), 0
        else:                                     # bottom right
            x1a, y1a, x2a, y2a = xc, yc, min(xc + w, S * 2), min(S * 2, yc + h)
            x1b, y1b = 0, 0
        out[i] = x1a, y1a, x2a, y2a, x1a - x1b, y1a - y1b
    return out


def fill_mosaic_layer(layer, m, sizes, tiles):
    """One layer of an adaisp_mosaic_u8 record (a MOSAIC_LAYER element), all but the tiles' src_offset: the Q16 map `m` of
    fixed_inverse, and per tile its source's (h, w) from `sizes` and its row (x0, y0, x1, y1, dx, dy) of mosaic_tiles."""
    layer["m"], layer["n_tiles"] = m, len(tiles)
    for t, (h, w), row in zip(layer["tile"], sizes, tiles):
        t["h"], t["w"] = h, w
        t["x0"], t["y0"], t["x1"], t["y1"], t["dx"], t["dy"] = row


def fill_single_layer(layer, m, h, w, top, left):
    """The layer of one h x w image letterboxed at (top, left): adaisp_augment_u8's image as one tile that covers
    [left, left + w) x [top, top + h) with (dx, dy) = (left, top)."""
    fill_mosaic_layer(layer, m, [(h, w)], [(left, top, left + w, top + h, left, top)])


def mosaic_boxes(labels, sizes, tiles, M, s, S):
    """The label rows of one mosaic after its warp: `labels`: per tile the image's own rows [k,5] (class, x, y, w, h
    normalised to the image), `sizes` their (h, w), `tiles` of mosaic_tiles. Per tile xywhn2xyxy(rows, w, h, padw, padh);
    the tiles' rows concatenated and clipped to [0, 2 S]; then warp_boxes. Returns class + pixel xyxy in the S x S frame,
    float64: what `mixup` concatenates and finish_labels ends."""
    rows = []
    for lb, (h, w), t in zip(labels, sizes, tiles):
        lb = np.array(lb, np.float64).reshape(-1, 5)
        box = lb.copy()
        box[:, 1] = w * (lb[:, 1] - lb[:, 3] / 2) + t[4]
        box[:, 2] = h * (lb[:, 2] - lb[:, 4] / 2) + t[5]
        box[:, 3] = w * (lb[:, 1] + lb[:, 3] / 2) + t[4]
        box[:, 4] = h * (lb[:, 2] + lb[:, 4] / 2) + t[5]
        rows.append(box)
    rows = np.concatenate(rows) if rows else np.zeros((0, 5))
    rows[:, 1:] = rows[:, 1:].clip(0, 2 * S)
    return warp_boxes(rows, M, s, S)


def mix_q16(r):
    """The mixup ratio r = nprs.beta(32, 32) as adaisp_mosaic_u8's weight of the first mosaic: rint(65536 r)."""
    return int(np.rint(65536.0 * r))
