"""numpy restatement of adaisp_resize_u8's arithmetic (csrc/isp_resize.hip), applied through the host tap tables of
adaptiveisp_amd/resize.py: integer math for LINEAR and AREA_INT, and for AREA each tap one fp32 multiply then one fp32 add
in source order, horizontal pass then vertical pass, round half to even, clip. The tests hold it against the host path
(val/loader.py) on the CPU and against the kernel on the GPU."""
import numpy as np

from adaptiveisp_amd import _lib
from adaptiveisp_amd.resize import area_int_scale, area_table, choose_mode, linear_table


def _csr(t, n):
    ptr = t[:n + 1].astype(np.int64)
    nnz = int(ptr[-1])
    return ptr, t[n + 1:n + 1 + nnz].astype(np.int64), t[n + 1 + nnz:n + 1 + 2 * nnz].view(np.float32)


def _sequential(img, t, n, axis):
    """out[.., d, ..] = sum over the CSR taps of d, in order, of weight * img[.., idx, ..]: fp32, mul then add."""
    ptr, idx, wt = _csr(t, n)
    cnt = np.diff(ptr)
    shape = list(img.shape)
    shape[axis] = n
    out = np.zeros(shape, np.float32)
    for k in range(int(cnt.max())):
        d = np.nonzero(cnt > k)[0]
        j = idx[ptr[d] + k]
        w = wt[ptr[d] + k]
        if axis == 1:
            out[:, d] = out[:, d] + w[None, :, None] * np.take(img, j, axis=1)
        else:
            out[d] = out[d] + w[:, None, None] * np.take(img, j, axis=0)
    return out


def resize_ref(img, dst_hw, area):
    """img HWC uint8 -> (h, w) by the mode choose_mode gives; `area` as in resize.choose_mode."""
    H, W = img.shape[:2]
    h, w = int(dst_hw[0]), int(dst_hw[1])
    mode = choose_mode((H, W), (h, w), area)
    if mode == _lib.RESIZE_COPY:
        return img.copy()
    if mode == _lib.RESIZE_LINEAR:
        x0, x1, a0, a1 = linear_table(W, w).reshape(4, w)
        y0, y1, b0, b1 = linear_table(H, h).reshape(4, h)
        s = img.astype(np.int32)
        rows = s[:, x0] * a0[None, :, None] + s[:, x1] * a1[None, :, None]
        top, bot = rows[y0] >> 4, rows[y1] >> 4
        out = (((b0[:, None, None] * top) >> 16) + ((b1[:, None, None] * bot) >> 16) + 2) >> 2
        return np.clip(out, 0, 255).astype(np.uint8)
    if mode == _lib.RESIZE_AREA_INT:
        fx, fy = W // w, H // h
        blk = img.astype(np.int64).reshape(h, fy, w, fx, -1).sum(axis=(1, 3))
        if fx == 2 and fy == 2:
            return ((blk + 2) >> 2).astype(np.uint8)
        return np.clip(np.rint(blk.astype(np.float32) * area_int_scale((H, W), (h, w))), 0, 255).astype(np.uint8)
    tmp = _sequential(img.astype(np.float32), area_table(W, w), w, axis=1)
    acc = _sequential(tmp, area_table(H, h), h, axis=0)
    return np.clip(np.rint(acc), 0, 255).astype(np.uint8)


def photo(h, w, seed):
    """A seeded uint8 HWC image with smooth content and noise (what the tests resample)."""
    rs = np.random.RandomState(seed)
    yy, xx = np.mgrid[0:h, 0:w].astype(np.float32)
    f = rs.uniform(0.005, 0.05, 3)
    im = np.stack([127 + 120 * np.sin(f[c] * xx + f[(c + 1) % 3] * yy + c) for c in range(3)], -1)
    return np.clip(im + rs.normal(0, 12, im.shape), 0, 255).astype(np.uint8)
