"""Float64 restatements of the eval policy kernels' layers (csrc/isp_policy.hip: k_trunk_mfma / k_trunk_conv, k_fc1), host only.

Each function returns the layer's output and, per output element, the magnitude sum A = sum |in| * |w| + |bias| that the
summation-error bounds of tests/test_gpu_policy_kernels.py scale with. tests/test_policyref_host.py pins these functions to the
PyTorch modules in double precision before the device is compared with them. Test infrastructure only."""
import numpy as np

SLOPE = 0.2        # nn.LeakyReLU(negative_slope=0.2)


def lrelu(v, slope=SLOPE):
    """LeakyReLU in the dtype of v (float64 for the reference; float32 restates the kernels' `v > 0 ? v : 0.2f * v`)."""
    v = np.asarray(v)
    return np.where(v > 0, v, v.dtype.type(slope) * v)


def _patches(x, Ho):
    """x [..., C, H, H] -> [..., C*16, Ho*Ho]: row ci*16 + kh*4 + kw holds x[ci, 2oy-1+kh, 2ox-1+kw], zero outside the frame."""
    lead, (C, H) = x.shape[:-3], x.shape[-3:-1]
    xp = np.zeros(lead + (C, H + 2, H + 2), dtype=np.float64)
    xp[..., 1:H + 1, 1:H + 1] = x
    taps = [xp[..., kh:kh + 2 * Ho:2, kw:kw + 2 * Ho:2] for kh in range(4) for kw in range(4)]     # each [..., C, Ho, Ho]
    return np.stack(taps, axis=-3).reshape(lead + (C * 16, Ho * Ho))


def trunk_conv(inp, states, w, bias, act=True):
    """Conv2d(kernel 4, stride 2, padding 1) + LeakyReLU(0.2) of G trunks: out[g,b,co,oy,ox] = lrelu(bias[g,co] +
    sum_{ci,kh,kw} in[g,b,ci,2oy-1+kh,2ox-1+kw] * w[g,co,ci,kh,kw]).

    `states` None: inp is [G,B,Cin,H,H]. `states` [B,S]: the first layer, inp is the image [B,3,H,H] that every trunk shares and
    the state vector follows as S constant planes (enrich_image_input) — constant INSIDE the frame, zero in the padding like the
    image. w [G,Cout,Cin,4,4], bias [G,Cout]. Returns (out, A), both float64 [G,B,Cout,H/2,H/2]; act=False leaves the
    pre-activation."""
    inp, w, bias = (np.asarray(a, dtype=np.float64) for a in (inp, w, bias))
    G, Cout, Cin = w.shape[:3]
    H = inp.shape[-1]
    Ho = H // 2
    if states is not None:
        states = np.asarray(states, dtype=np.float64)
        B = inp.shape[0]
        assert inp.shape == (B, 3, H, H) and states.shape == (B, Cin - 3)
        planes = np.broadcast_to(states[:, :, None, None], (B, Cin - 3, H, H))
        x = np.concatenate([inp, planes], axis=1)[None]                      # [1,B,Cin,H,H]: shared by the trunks
    else:
        B = inp.shape[1]
        assert inp.shape == (G, B, Cin, H, H)
        x = inp
    p = _patches(x, Ho)                                                      # [G or 1, B, K, P]
    wk = w.reshape(G, 1, Cout, Cin * 16)
    pre = np.matmul(wk, p) + bias[:, None, :, None]                          # [G,B,Cout,P]
    A = np.matmul(np.abs(wk), np.abs(p)) + np.abs(bias)[:, None, :, None]
    shape = (G, B, Cout, Ho, Ho)
    return (lrelu(pre) if act else pre).reshape(shape), A.reshape(shape)


def fc1(feats, head_src, w1, b1, act=True):
    """hidden[b,h,j] = lrelu(b1[h,j] + feats[head_src[h],b,:] . w1[h,j,:]); feats [S,B,D], w1 [NH,HID,D], b1 [NH,HID].
    Returns (hidden, A), float64 [B,NH,HID]."""
    feats, w1, b1 = (np.asarray(a, dtype=np.float64) for a in (feats, w1, b1))
    f = feats[np.asarray(head_src, dtype=np.int64)]                          # [NH,B,D]
    pre = np.matmul(f, w1.transpose(0, 2, 1)) + b1[:, None, :]               # [NH,B,HID]
    A = np.matmul(np.abs(f), np.abs(w1).transpose(0, 2, 1)) + np.abs(b1)[:, None, :]
    return (lrelu(pre) if act else pre).transpose(1, 0, 2), A.transpose(1, 0, 2)


def lattice(rng, shape, step, lim, signed=True):
    """float32 values k * step with |k * step| <= lim, k uniform over the integers that allows (k >= 0 when not signed). With
    step a power of two every value, and every product of two of them, is exact in float32."""
    n = int(np.floor(lim / step + 1e-9))
    k = rng.integers(-n if signed else 0, n + 1, size=shape)
    return (k.astype(np.float64) * step).astype(np.float32)
