"""SPP's three max pools (5, 9, 13; stride 1, padding k // 2) and their gradient restated in numpy float64 — what
adayolo_spp_fwd / adayolo_spp_bwd (include/adayolo.h) are tested against. NHWC, like the kernels.

The gradient of a pool goes to the FIRST maximum of each clipped window in row-major order (strict >), which is how torch's
max_pool2d routes it (tests/test_spp_host.py checks this restatement against torch-CPU, ties included). Test infrastructure only."""
import numpy as np

KS = (5, 9, 13)


def _windows(x, k):
    """x [B,H,W,C] -> [B,H,W,C,k*k]: every pixel's k x k window in row-major order, -inf outside the map."""
    h = k // 2
    xp = np.pad(np.asarray(x, np.float64), ((0, 0), (h, h), (h, h), (0, 0)), constant_values=-np.inf)
    w = np.lib.stride_tricks.sliding_window_view(xp, (k, k), axis=(1, 2))          # [B,H,W,C,k,k]
    return w.reshape(*w.shape[:4], k * k)


def forward(x):
    """x [B,H,W,C] -> [B,H,W,3C] float64: channels [0,C) the 5x5 max, [C,2C) 9x9, [2C,3C) 13x13."""
    return np.concatenate([_windows(x, k).max(-1) for k in KS], -1)


def backward(x, grad_out):
    """x [B,H,W,C], grad_out [B,H,W,3C] -> (grad_x [B,H,W,C] float64, S: the sum of |contributions| per element)."""
    x = np.asarray(x, np.float64)
    go = np.asarray(grad_out, np.float64)
    B, H, W, C = x.shape
    gx, S = np.zeros_like(x), np.zeros_like(x)
    b, y, xx, c = np.meshgrid(np.arange(B), np.arange(H), np.arange(W), np.arange(C), indexing="ij")
    for i, k in enumerate(KS):
        h = k // 2
        first = _windows(x, k).argmax(-1)                     # numpy's argmax returns the first maximum
        ty, tx = y + first // k - h, xx + first % k - h
        assert (ty >= 0).all() and (ty < H).all() and (tx >= 0).all() and (tx < W).all()
        g = go[..., i * C:(i + 1) * C]
        np.add.at(gx, (b, ty, tx, c), g)
        np.add.at(S, (b, ty, tx, c), np.abs(g))
    return gx, S
