"""numpy definition of adaisp_raw_load (include/adaisp.h), composed from the restatements the tests already have: the
demosaic of the whole plane (_mhcref.mhc; _bayerref.demosaic_rect with the plane as its own rectangle), the fp32 gain
multiply, _resizeref._sequential over raw_table(W, w) on axis 1 and then over raw_table(H, h) on axis 0 (one fp32
multiply then one fp32 add per tap, in tap order, from 0), and the placement into zeros. It defines the output bit for
bit; `exact` is the float64 product of the same fp32 weights, against which tests/test_raw_load_host.py bounds it."""
import numpy as np

import _bayerref
import _mhcref
import _resizeref
from adaptiveisp_amd.resize import raw_table

CFA = _mhcref.CFA


def demosaic(plane, pattern="RGGB", method="mhc", black=0.0, white=65535.0):
    """fp32 [3, H, W] of a uint16 [H, W] plane, H, W >= 2 of any parity."""
    H, W = plane.shape
    if method == "mhc":
        return _mhcref.mhc(plane, pattern, black, white)
    side = max(H, W)
    frame = np.zeros((side, side), np.uint16)
    frame[:H, :W] = plane
    return _bayerref.demosaic_rect(frame, H, W, 0, 0, pattern, black, white)[:, :H, :W]


def resample(chw, h, w, tx=None, ty=None):
    """[3, H, W] fp32 -> [3, h, w] through raw_table (or the CSR tables given), horizontal pass then vertical pass."""
    _, H, W = chw.shape
    hwc = np.ascontiguousarray(chw.transpose(1, 2, 0)).astype(np.float32)
    t = _resizeref._sequential(hwc, raw_table(W, w) if tx is None else tx, w, axis=1)
    t = _resizeref._sequential(t, raw_table(H, h) if ty is None else ty, h, axis=0)
    return np.ascontiguousarray(t.transpose(2, 0, 1))


def raw_load_one(plane, hw, place, S, pattern="RGGB", method="mhc", black=0.0, white=65535.0, gains=None, tx=None, ty=None):
    """One image of adaisp_raw_load: fp32 [3, S, S]. A plane with a side under 2, or a placement that does not fit the
    frame, gives zeros. gains None: no multiply at all. tx, ty: CSR tables other than raw_table's."""
    (h, w), (top, left) = hw, place
    out = np.zeros((3, S, S), np.float32)
    if plane.ndim != 2 or min(plane.shape) < 2 or h < 1 or w < 1 or top < 0 or left < 0 or top + h > S or left + w > S:
        return out
    d = demosaic(plane, pattern, method, black, white)
    if gains is not None:
        d = d * np.asarray(gains, np.float32)[:, None, None]
    out[:, top:top + h, left:left + w] = resample(d, h, w, tx, ty)
    return out


def _dense(t, n, src):
    ptr, idx, wt = _resizeref._csr(t, n)
    m = np.zeros((n, src), np.float64)
    for d in range(n):
        for k in range(ptr[d], ptr[d + 1]):
            m[d, idx[k]] += np.float64(wt[k])
    return m


def exact(d_chw, h, w):
    """float64 [3, h, w]: the product of the same fp32 weights with the fp32 values d_chw, without intermediate rounding."""
    _, H, W = d_chw.shape
    mx, my = _dense(raw_table(W, w), w, W), _dense(raw_table(H, h), h, H)
    return np.einsum("yj,cji,xi->cyx", my, d_chw.astype(np.float64), mx)


def max_taps(src, dst):
    ptr = _resizeref._csr(raw_table(src, dst), dst)[0]
    return int(np.diff(ptr).max())


def plane(h, w, seed, black=64, white=4095):
    """A seeded uint16 [h, w] plane with smooth content and noise inside black .. white."""
    rs = np.random.RandomState(seed)
    yy, xx = np.mgrid[0:h, 0:w].astype(np.float64)
    v = 0.5 + 0.45 * np.sin(0.07 * xx + 0.05 * yy + seed) + rs.normal(0, 0.04, (h, w))
    return np.clip(np.rint(black + np.clip(v, 0, 1) * (white - black)), 0, 65535).astype(np.uint16)
