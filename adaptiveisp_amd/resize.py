"""Host half of the device resampler (adaisp_resize_u8, csrc/isp_resize.hip): which of load_image's / letterbox's
branches an image takes, and the tap tables the kernel reads. The tables are the host path's own numbers
(val/loader.py: `_linear_taps`, the nonzeros of `_area_weights`, the fast-area factor float32(1 / (fx fy))), so the
device computes nothing about weights in floating point.

Table layout (32-bit words; floats by their bits), per (source size, destination size) along one axis:
  LINEAR  i0[n], i1[n], w0[n], w1[n]
  AREA    ptr[n + 1], idx[nnz], weight[nnz]   (CSR over the destination index, source order; nnz = ptr[n])

The raw-capture loader (adaisp_raw_load, csrc/isp_raw_load.hip) resamples fp32 values and reads every table in the AREA
layout: `raw_table` gives it the area weights when shrinking, `linear_table_f32` when enlarging and the identity when the
sizes are equal; `RawTapPlan` lays out its descriptors and tables.
"""
import functools

import numpy as np

from ._lib import RAW_DESC, RESIZE_AREA, RESIZE_AREA_INT, RESIZE_COPY, RESIZE_DESC, RESIZE_LINEAR
from .val.loader import _area_weights, _linear_taps


def choose_mode(src_hw, dst_hw, area):
    """The branch the host path takes from (H, W) to (h, w): `area` = resize_area_u8 (load_image shrinking for
    evaluation), otherwise resize_linear_u8 (load_image enlarging, letterbox's resize)."""
    (H, W), (h, w) = src_hw, dst_hw
    if (W, H) == (w, h):
        return RESIZE_COPY
    if not area or w > W or h > H:
        return RESIZE_LINEAR
    if W % w == 0 and H % h == 0:
        return RESIZE_AREA_INT
    return RESIZE_AREA


@functools.lru_cache(maxsize=256)
def linear_table(src, dst):
    """_linear_taps(src, dst) as one int32 array: i0, i1, w0, w1 (dst words each)."""
    i0, i1, w0, w1 = _linear_taps(src, dst)
    t = np.concatenate([i0, i1, w0, w1]).astype(np.int32)
    t.flags.writeable = False
    return t


@functools.lru_cache(maxsize=256)
def area_table(src, dst):
    """The nonzeros of _area_weights(src, dst) as CSR in source order: ptr[dst + 1], idx[nnz], the fp32 weights' bits."""
    m = _area_weights(src, dst)
    rows, cols = np.nonzero(m)                        # row-major: every row's columns ascending
    ptr = np.zeros(dst + 1, np.int64)
    np.add.at(ptr, rows + 1, 1)
    t = np.concatenate([np.cumsum(ptr), cols, m[rows, cols].astype(np.float32).view(np.int32)]).astype(np.int32)
    t.flags.writeable = False
    return t


def _csr(counts, idx, weights):
    t = np.concatenate([np.concatenate([[0], np.cumsum(counts)]), idx, np.asarray(weights, np.float32).view(np.int32)])
    t = t.astype(np.int32)
    t.flags.writeable = False
    return t


@functools.lru_cache(maxsize=256)
def linear_table_f32(src, dst):
    """Bilinear taps with fp32 weights as CSR (the AREA layout): the pixel-centre mapping and edge rules of _linear_taps,
    `frac` kept in fp32 instead of 11 bits; per row the taps (i0, 1 - frac), (i0 + 1, frac), or the single tap (i0, 1)
    where frac == 0 (an exact hit, and both clamped edges)."""
    scale = src / dst
    f = (np.arange(dst, dtype=np.float64) + 0.5) * scale - 0.5
    i0 = np.floor(f).astype(np.int64)
    frac = (f - i0).astype(np.float32)
    frac[i0 < 0] = 0.0
    i0 = np.maximum(i0, 0)
    edge = i0 >= src - 1
    frac[edge] = 0.0
    i0[edge] = src - 1
    two = frac != 0
    idx = np.stack([i0, i0 + 1], 1)[np.stack([np.ones(dst, bool), two], 1)]
    wt = np.stack([np.where(two, np.float32(1.0) - frac, np.float32(1.0)), frac], 1)[np.stack([np.ones(dst, bool), two], 1)]
    return _csr(1 + two.astype(np.int64), idx, wt)


@functools.lru_cache(maxsize=256)
def identity_table(n):
    """One tap of weight 1 per row, as CSR."""
    return _csr(np.ones(n, np.int64), np.arange(n), np.ones(n, np.float32))


def raw_table(src, dst):
    """The CSR taps adaisp_raw_load resamples one axis with: the area weights when shrinking, fp32 bilinear when
    enlarging, the identity when the sizes are equal."""
    src, dst = int(src), int(dst)
    if dst < src:
        return area_table(src, dst)
    return linear_table_f32(src, dst) if dst > src else identity_table(src)


def area_int_scale(src_hw, dst_hw):
    """resize_area_u8's fast-area factor float32(1 / (fx * fy)) (unused for 2 x 2 blocks, which round with (sum + 2) >> 2)."""
    (H, W), (h, w) = src_hw, dst_hw
    return np.float32(1.0 / ((W // w) * (H // h)))


class TapPlan:
    """Descriptors and tap tables of one adaisp_resize_u8 call. add() one image at a time; tables shared by images with
    the same (kind, source size, destination size) are stored once. `base` is the word offset of the table block in the
    buffer the kernel gets as `tabs`."""

    def __init__(self, base=0):
        self.base = int(base)
        self.records = []
        self.chunks = []
        self.words = 0
        self._at = {}

    def _table(self, kind, src, dst):
        key = (kind, src, dst)
        if key not in self._at:
            t = linear_table(src, dst) if kind == RESIZE_LINEAR else area_table(src, dst)
            self._at[key] = self.base + self.words
            self.chunks.append(t)
            self.words += t.size
        return self._at[key]

    def add(self, src_hw, dst_hw, area, src_offset, dst_offset):
        """Image (H, W) at byte `src_offset` of src -> (h, w) at byte `dst_offset` of dst; returns its mode."""
        (H, W), (h, w) = (int(v) for v in src_hw), (int(v) for v in dst_hw)
        mode = choose_mode((H, W), (h, w), area)
        r = np.zeros((), RESIZE_DESC)
        r["src_offset"], r["dst_offset"], r["mode"] = src_offset, dst_offset, mode
        r["src_h"], r["src_w"], r["dst_h"], r["dst_w"] = H, W, h, w
        if mode in (RESIZE_LINEAR, RESIZE_AREA):
            r["tab_x"], r["tab_y"] = self._table(mode, W, w), self._table(mode, H, h)
        elif mode == RESIZE_AREA_INT:
            r["scale"] = area_int_scale((H, W), (h, w))
        self.records.append(r)
        return mode

    def descriptors(self):
        return np.array(self.records, RESIZE_DESC).reshape(-1)

    def table(self):
        return np.concatenate(self.chunks) if self.chunks else np.zeros(0, np.int32)


class RawTapPlan:
    """Descriptors and tap tables of one adaisp_raw_load call, after TapPlan: add() one plane at a time; tables shared by
    planes with the same (source size, destination size) along an axis are stored once. `base` is the word offset of the
    table block in the buffer the kernel gets as `tabs`."""

    def __init__(self, base=0):
        self.base = int(base)
        self.records = []
        self.chunks = []
        self.words = 0
        self._at = {}

    def _table(self, src, dst):
        key = (src, dst)
        if key not in self._at:
            t = raw_table(src, dst)
            self._at[key] = self.base + self.words
            self.chunks.append(t)
            self.words += t.size
        return self._at[key]

    def add(self, src_hw, dst_hw, place, src_offset, gains=(1.0, 1.0, 1.0)):
        """Plane (H, W) at byte `src_offset` of src -> (h, w) at `place` = (top, left) of its frame."""
        (H, W), (h, w) = (int(v) for v in src_hw), (int(v) for v in dst_hw)
        r = np.zeros((), RAW_DESC)
        r["src_offset"], r["src_h"], r["src_w"], r["h"], r["w"] = src_offset, H, W, h, w
        r["top"], r["left"], r["gain"] = int(place[0]), int(place[1]), np.asarray(gains, np.float32)
        r["tab_x"], r["tab_y"] = self._table(W, w), self._table(H, h)
        self.records.append(r)

    def descriptors(self):
        return np.array(self.records, RAW_DESC).reshape(-1)

    def table(self):
        return np.concatenate(self.chunks) if self.chunks else np.zeros(0, np.int32)
