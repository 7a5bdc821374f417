"""Host half of the device resampler (adaisp_resize_u8, csrc/isp_resize.hip): which of load_image's / letterbox's
branches an image takes, and the tap tables the kernel reads. The tables are the host path's own numbers
(val/loader.py: `_linear_taps`, the nonzeros of `_area_weights`, the fast-area factor float32(1 / (fx fy))), so the
device computes nothing about weights in floating point.

Table layout (32-bit words; floats by their bits), per (source size, destination size) along one axis:
  LINEAR  i0[n], i1[n], w0[n], w1[n]
  AREA    ptr[n + 1], idx[nnz], weight[nnz]   (CSR over the destination index, source order; nnz = ptr[n])
"""
import functools

import numpy as np

from ._lib import RESIZE_AREA, RESIZE_AREA_INT, RESIZE_COPY, RESIZE_DESC, RESIZE_LINEAR
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
