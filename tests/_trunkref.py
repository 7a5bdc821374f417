"""Float64 restatements of the training-mode trunk kernels (csrc/isp_trunk_train.hip), stage by stage, host only, numpy.

One function per stage: conv (k_tconv_fwd), bn_fwd / bn_apply / running (k_tbn_fwd), bn_bwd (k_tbn_bwd), wgrad (k_twgrad +
k_twgrad_reduce), dgrad (k_tdgrad), plane_sum (k_tplane_sum); each returns the value and the magnitude sum A = sum |terms| per
output that its summation bound scales with. `plan` restates the library's private buffer layout (make_plan), `geometry` the
launch geometry the host code picks from B and C, `chain` composes the stages forward and backward, CASES is the case list that
tests/test_trunkref_host.py and tests/test_gpu_trunk_stages.py share, and `stage_shares` is the stage-by-stage check both run:
every stage of a set of buffers (the device's, or a float32 restatement's) against the float64 stage function applied to THOSE
buffers' own upstream values, as a share of a bound derived from u = 2^-24, the kernel's longest addition chain K and A.
tests/test_trunkref_host.py pins chain to nets.FeatureExtractor under float64 autograd. Test infrastructure only."""
import math

import numpy as np

import _policyref as P

LAYERS = 4
U = 2.0 ** -24
KU = 8                  # kU of isp_trunk_train.hip: channels per slice step
PER_THREAD = 8          # kPerThread
MAX_WSPLIT = 8          # kMaxWSplit
CHUNK = 32              # images per step of the float64 GEMMs (B = 513 stays within a few hundred MB)


def f32(v):
    """The double that equals the float32 the device receives (momentum, eps, slope are floats in adaisp_trunk_args)."""
    return float(np.float32(v))


# ---- layout and launch geometry, restating the host code ---------------------------------------------------------------------------
def plan(B, C, G):
    """make_plan: float offsets of y, a, mean, rstd in one instance's workspace block and of dy, da in its scratch block (index
    l = 1..4; a[4] is `feat`, da[4] is `dfeat`, da[0] holds the first layer's state-plane gradients), the per-instance totals,
    and the weight-gradient partial region that follows the G scratch blocks."""
    H = [64 >> l for l in range(LAYERS + 1)]
    p = dict(H=H, y={}, a={}, mean={}, rstd={}, dy={}, da={})
    o = s = 0
    for l in range(1, LAYERS + 1):
        n = B * C[l] * H[l] * H[l]
        p["y"][l] = o; o += n
        if l < LAYERS:
            p["a"][l] = o; o += n
        p["mean"][l] = o; o += (C[l] + 3) & ~3
        p["rstd"][l] = o; o += (C[l] + 3) & ~3
        p["dy"][l] = s; s += n
        if l < LAYERS:
            p["da"][l] = s; s += n
    p["da"][0] = s; s += B * C[0] * 64 * 64
    p["ws_per_g"], p["scr_per_g"], p["wpart"] = o, s, s * G
    wp = 0
    for l in range(1, LAYERS + 1):
        PS = wgrad_chunks(B * H[l] * H[l] // 16)
        wp = max(wp, PS * G * C[l] * C[l - 1] * 16 if PS > 1 else 0)
    p["wpart_size"], p["ws_total"], p["scr_total"] = wp, o * G, s * G + wp
    return p


def wgrad_chunks(steps):
    PS = 1
    while PS < MAX_WSPLIT and steps % (2 * PS) == 0 and steps // (2 * PS) >= 16 * 4:
        PS *= 2
    return PS


def _largest_divisor_le(n, cap):
    for k in range(cap, 1, -1):
        if n % k == 0:
            return k
    return 1


def geometry(B, C, Gseq=1):
    """{l: what adaisp_trunk_train_fwd / _bwd launch at layer l}: BatchNorm REG / STREAM, nthr and the length of its addition
    chain; the weight gradient's PS / KS / spw / U; the conv's KS / cpw / padded channels / wholly masked waves; the data
    gradient's KS / cpw."""
    out = {}
    for l in range(1, LAYERS + 1):
        Cin, Cout, Ho = C[l - 1], C[l], 64 >> l
        N = B * Ho * Ho
        nthr = ((N + 63) & ~63) if N < 1024 else 1024
        reg = N <= 1024 * PER_THREAD
        trips, nw = -(-N // nthr), nthr // 64
        steps = N // 16
        PS = wgrad_chunks(steps)
        per = steps // PS
        wKS = _largest_divisor_le(per, 16)
        spw = per // wKS
        cKS = min(16, -(-Cin // KU))
        ccpw = -(-Cin // (cKS * KU)) * KU
        dKS = min(16, Cout // KU)
        while Cout % (dKS * KU):
            dKS -= 1
        out[l] = dict(N=N, bn="REG" if reg else "STREAM", nthr=nthr, trips=trips, nw=nw, bn_K=trips + 6 + nw,
                      PS=PS, wKS=wKS, spw=spw, U=4 if spw % 4 == 0 else 2 if spw % 2 == 0 else 1,
                      nsplit=Gseq * PS if PS > 1 else 1, w_K=16 * spw * (Gseq if PS == 1 else 1) + wKS + (Gseq * PS if PS > 1 else 1),
                      cKS=cKS, ccpw=ccpw, cpad=cKS * ccpw - Cin, cmasked=sum(1 for k in range(cKS) if k * ccpw >= Cin),
                      dKS=dKS, dcpw=Cout // dKS)
    return out


def geometry_table():
    """The docstring table of tests/test_gpu_trunk_stages.py (tests/test_trunkref_host.py asserts the two are equal)."""
    lines = []
    for c in CASES:
        geo = geometry(c["B"], c["C"], c["G"] if c["share"] else 1)
        lines.append(f"  {c['name']}")
        for l, g in geo.items():
            lines.append(f"    L{l} bn {g['bn']} nthr {g['nthr']} N {g['N']} | wgrad PS {g['PS']} KS {g['wKS']} spw {g['spw']} U {g['U']} | "
                         f"conv KS {g['cKS']} cpw {g['ccpw']} pad {g['cpad']} masked waves {g['cmasked']} | dgrad KS {g['dKS']} "
                         f"cpw {g['dcpw']}")
    return "\n".join(lines)


# ---- the stages in float64 -----------------------------------------------------------------------------------------------------------
def _full_input(img, svec):
    """[B,3,H,H] + [B,S] -> [B,3+S,H,H]: the state vector as constant planes (zero-padded by the conv like any other channel)."""
    img = np.asarray(img, dtype=np.float64)
    if svec is None or np.asarray(svec).shape[1] == 0:
        return img
    sv = np.asarray(svec, dtype=np.float64)
    return np.concatenate([img, np.broadcast_to(sv[:, :, None, None], sv.shape + img.shape[2:])], axis=1)


def conv(a_in, w, bias, svec=None):
    """y[b,co,oy,ox] = bias[co] + sum_{ci,kh,kw} in[b,ci,2oy-1+kh,2ox-1+kw] w[co,ci,kh,kw]; a_in is the previous activation
    [B,Cin,H,H], or with `svec` the image [B,3,H,H]. -> (y, A)."""
    x = _full_input(a_in, svec)
    w, bias = np.asarray(w, dtype=np.float64)[None], np.asarray(bias, dtype=np.float64)[None]
    ys, As = [], []
    for b0 in range(0, x.shape[0], CHUNK):
        y, A = P.trunk_conv(x[None, b0:b0 + CHUNK], None, w, bias, act=False)
        ys.append(y[0]); As.append(A[0])
    return np.concatenate(ys), np.concatenate(As)


def bn_fwd(y, gamma, beta, eps, slope):
    """BatchNorm2d with batch statistics + LeakyReLU -> mean, var (biased), rstd, a."""
    y = np.asarray(y, dtype=np.float64)
    mean = y.mean(axis=(0, 2, 3))
    var = ((y - mean[None, :, None, None]) ** 2).mean(axis=(0, 2, 3))
    rstd = 1.0 / np.sqrt(var + eps)
    return mean, var, rstd, bn_apply(y, mean, rstd, gamma, beta, slope)[0]


def bn_apply(y, mean, rstd, gamma, beta, slope):
    """a = lrelu((y - mean) rstd gamma + beta) with mean and rstd as given -> (a, z, T); T = |(y - mean) rstd gamma| + |beta|."""
    c = lambda v: np.asarray(v, dtype=np.float64)[None, :, None, None]  # noqa: E731
    t = (np.asarray(y, dtype=np.float64) - c(mean)) * c(rstd) * c(gamma)
    z = t + c(beta)
    return np.where(z > 0, z, z * slope), z, np.abs(t) + np.abs(c(beta))


def running(r_mean, r_var, stats, N, momentum):
    """nn.BatchNorm2d's update, once per instance in instance order: stats = [(mean, biased var)], the variance made unbiased
    with N / (N - 1)."""
    r_mean, r_var = np.asarray(r_mean, dtype=np.float64), np.asarray(r_var, dtype=np.float64)
    for mean, var in stats:
        r_mean = (1.0 - momentum) * r_mean + momentum * mean
        r_var = (1.0 - momentum) * r_var + momentum * (var * N / (N - 1))
    return r_mean, r_var


def bn_bwd(da, mask, y, mean, rstd, gamma, slope):
    """Backward of bn_apply: d = da (mask) or slope da, x = (y - mean) rstd, dy = (d - mean(d) - x mean(d x)) gamma rstd;
    dbeta = sum d, dgamma = sum d x, dbias = sum dy (0 in exact arithmetic when mean is y's own). -> dict with the magnitude
    sums A1 = sum |d|, A2 = sum |d x| and the element-wise pieces the dy bound is made of."""
    c = lambda v: np.asarray(v, dtype=np.float64)[None, :, None, None]  # noqa: E731
    da, y = np.asarray(da, dtype=np.float64), np.asarray(y, dtype=np.float64)
    d = np.where(mask, da, da * slope)
    x = (y - c(mean)) * c(rstd)
    ax = (0, 2, 3)
    N = y.shape[0] * y.shape[2] * y.shape[3]
    s1, s2 = d.sum(axis=ax), (d * x).sum(axis=ax)
    k0 = np.asarray(gamma, dtype=np.float64) * np.asarray(rstd, dtype=np.float64)
    dy = (d - c(s1 / N) - x * c(s2 / N)) * c(k0)
    return dict(dy=dy, dbeta=s1, dgamma=s2, dbias=dy.sum(axis=ax), A1=np.abs(d).sum(axis=ax), A2=np.abs(d * x).sum(axis=ax),
                d=d, x=x, m1=s1 / N, m2=s2 / N, k0=k0, N=N)


def wgrad(dy, a_in, svec=None):
    """dW[co,ci,kh,kw] = sum_{b,oy,ox} dy[b,co,oy,ox] in[b,ci,2oy-1+kh,2ox-1+kw] -> (dW, A)."""
    x = _full_input(a_in, svec)
    dy = np.asarray(dy, dtype=np.float64)
    B, Cout, Ho = dy.shape[:3]
    Cin = x.shape[1]
    dW, A = np.zeros((Cout, Cin * 16)), np.zeros((Cout, Cin * 16))
    for b0 in range(0, B, CHUNK):
        p = P._patches(x[b0:b0 + CHUNK], Ho)                                                # [b, K, P]
        d = dy[b0:b0 + CHUNK].reshape(-1, Cout, Ho * Ho)
        dW += np.matmul(d, p.transpose(0, 2, 1)).sum(axis=0)
        A += np.matmul(np.abs(d), np.abs(p).transpose(0, 2, 1)).sum(axis=0)
    return dW.reshape(Cout, Cin, 4, 4), A.reshape(Cout, Cin, 4, 4)


def parity_taps(ry, rx):
    """The 2 x 2 taps that reach input pixels of parity (ry, rx): [(kh, kw, dy row shift, dy column shift)]; input pixel
    (2u + ry, 2v + rx) receives tap (kh, kw) from output pixel (u + shift_y, v + shift_x)."""
    return [(((ry + 1) & 1) + 2 * a, ((rx + 1) & 1) + 2 * c, ry - a, rx - c) for a in range(2) for c in range(2)]


def dgrad_terms(dy, w, ry, rx, dtype=np.float64, edge=None):
    """The operands of one parity class: D [B, Cout*4, Ho*Ho] (dy shifted per tap, zero outside the frame) and
    Wc [Cin, Cout*4]. `edge` = a tap index whose out-of-frame reads take the clamped pixel instead of zero (a mutant)."""
    dy = np.asarray(dy, dtype=dtype)
    w = np.asarray(w, dtype=dtype)
    B, Cout, Ho = dy.shape[:3]
    pad = np.zeros((B, Cout, Ho + 2, Ho + 2), dtype=dtype)
    pad[:, :, 1:-1, 1:-1] = dy
    rep = np.pad(dy, ((0, 0), (0, 0), (1, 1), (1, 1)), mode="edge") if edge is not None else None
    D, Wc = [], []
    for k, (kh, kw, sy, sx) in enumerate(parity_taps(ry, rx)):
        src = rep if edge == k else pad
        D.append(src[:, :, 1 + sy:1 + sy + Ho, 1 + sx:1 + sx + Ho])
        Wc.append(w[:, :, kh, kw])                                                           # [Cout, Cin]
    D = np.stack(D, axis=2).reshape(B, Cout * 4, Ho * Ho)
    Wc = np.stack(Wc, axis=1).reshape(Cout * 4, -1).T                                        # [Cin, Cout*4]
    return D, np.ascontiguousarray(Wc)


def dgrad(dy, w):
    """da_in[b,ci,iy,ix] = sum_{co,kh,kw} dy[b,co,(iy+1-kh)/2,(ix+1-kw)/2] w[co,ci,kh,kw] over the taps with integer output
    pixels inside the frame, by pixel parity -> (da_in, A), [B,Cin,2Ho,2Ho]."""
    B, Cout, Ho = np.asarray(dy).shape[:3]
    Cin = np.asarray(w).shape[1]
    out, A = np.zeros((B, Cin, 2 * Ho, 2 * Ho)), np.zeros((B, Cin, 2 * Ho, 2 * Ho))
    for b0 in range(0, B, CHUNK):
        for ry in range(2):
            for rx in range(2):
                D, Wc = dgrad_terms(np.asarray(dy)[b0:b0 + CHUNK], w, ry, rx)
                out[b0:b0 + CHUNK, :, ry::2, rx::2] = np.matmul(Wc[None], D).reshape(-1, Cin, Ho, Ho)
                A[b0:b0 + CHUNK, :, ry::2, rx::2] = np.matmul(np.abs(Wc)[None], np.abs(D)).reshape(-1, Cin, Ho, Ho)
    return out, A


def plane_sum(planes):
    """dsvec[b,s] = sum over plane s of image b -> (sum, A)."""
    p = np.asarray(planes, dtype=np.float64)
    return p.sum(axis=(2, 3)), np.abs(p).sum(axis=(2, 3))


# ---- cases and inputs ------------------------------------------------------------------------------------------------------------------
def _case(name, B, n_state, widths, G=1, share=False, n_in=1, want=(), special=False, momentum=0.1, eps=1e-5, slope=0.2,
          null_running=False):
    return dict(name=name, B=B, n_state=n_state, C=(3 + n_state,) + tuple(widths), G=G, share=share, n_in=n_in,
                want=tuple(g in want for g in range(G)), special=special, momentum=momentum, eps=eps, slope=slope,
                null_running=null_running)


PROD = (32, 64, 128, 256)
CASES = [
    _case("b1-two-sets", 1, 13, PROD, G=2),
    _case("b3-two-sets", 3, 13, PROD, G=2, special="zero"),
    _case("b5-shared", 5, 16, PROD, G=2, share=True, n_in=2, want=(1,)),
    _case("b7", 7, 13, PROD, momentum=0.3, eps=1e-3, slope=0.01),
    _case("b8-agent-pair", 8, 13, PROD, G=2, special="zero"),
    _case("b8-critic-pair", 8, 16, PROD, G=2, share=True, n_in=2, want=(0, 1)),
    _case("b9", 9, 13, PROD, special="zero"),
    _case("b17-shared", 17, 16, PROD, G=2, share=True, n_in=2, want=(0, 1)),
    _case("b33", 33, 13, PROD),
    _case("b129-narrow", 129, 0, (16, 32, 64, 128), want=(0,), special=True),
    _case("b513-narrow", 513, 0, (16, 32, 64, 128), special=True),
    _case("b4-wide", 4, 19, (48, 96, 192, 384), special="zero"),
    _case("b6-sixteen", 6, 0, (16, 16, 16, 16), null_running=True),
]
# special = True: the 1e3 offset channel and the all-zero channel; "zero": the all-zero channel alone. The offset channel sits in
# the two large batches, where a one-pass variance loses most and which the chain check leaves out: float32 carries a channel
# of mean 1e3 and spread < 1 with 4 digits fewer END TO END whatever the kernel does, the stage checks are not affected.
CHAIN_MAX_B = 33        # the chain check runs for B <= 33 (see tests/test_gpu_trunk_stages.py)


def param_set(c, g):
    return 0 if c["share"] else g


def inputs(c, seed=0):
    """float32 inputs of a case: img / svec per instance (one array twice when the instances share the input), the parameter
    sets, dfeat. Images in [-0.15, 1.15] with saturated 0 / 1 blocks and (B > 1) one constant image; `special` adds a layer-1
    channel with conv bias 1e3 (a large mean with a small spread) and a layer-2 channel with zero weights, zero bias and
    beta = 0 (its BatchNorm input is exactly 0: the activation and its gradient take the slope branch)."""
    rng = np.random.default_rng([11, seed, c["B"], c["C"][1]])
    B, S, C, G = c["B"], c["n_state"], c["C"], c["G"]
    f = np.float32
    imgs, svecs = [], []
    for _ in range(c["n_in"]):
        x = (rng.random((B, 3, 64, 64)) * 1.3 - 0.15).astype(f)
        x[:, :, :16, :16] = 1.0
        x[:, :2, 16:32, :16] = 1.0
        x[:, :, :16, 16:32] = 0.0
        if B > 1:
            x[B - 1] = 0.5
        imgs.append(x)
        svecs.append(rng.random((B, S)).astype(f) if S else None)
    if c["n_in"] == 1:
        imgs, svecs = imgs * G, svecs * G
    params = []
    for _ in range(1 if c["share"] else G):
        p = dict(w=[], bias=[], gamma=[], beta=[], rmean=[], rvar=[])
        for l in range(1, LAYERS + 1):
            p["w"].append((rng.normal(size=(C[l], C[l - 1], 4, 4)) / math.sqrt(16 * C[l - 1])).astype(f))
            p["bias"].append(rng.normal(0.0, 0.3, C[l]).astype(f))
            ga = rng.uniform(0.5, 1.5, C[l])
            ga[3::8] *= -1.0
            p["gamma"].append(ga.astype(f))
            p["beta"].append(rng.uniform(-0.3, 0.3, C[l]).astype(f))
            p["rmean"].append(rng.uniform(-0.2, 0.2, C[l]).astype(f))
            p["rvar"].append(rng.uniform(0.5, 2.0, C[l]).astype(f))
        if c["special"] is True:                                # ("zero": the all-zero channel alone)
            p["bias"][0][5] = 1e3
        if c["special"]:
            p["w"][1][7] = 0.0
            p["bias"][1][7] = 0.0
            p["beta"][1][7] = 0.0
        params.append(p)
    dfeat = rng.normal(size=(G, B, C[LAYERS], 4, 4)).astype(f)
    return dict(img=imgs, svec=svecs, params=params, dfeat=dfeat)


# ---- the stages composed --------------------------------------------------------------------------------------------------------------
def chain(c, t, masks=None, scalars=None):
    """The whole pass in float64 on the inputs `t` -> the buffers the device leaves, keyed like `stage_shares` reads them:
    ("y" | "a" | "mean" | "rstd" | "dy" | "da", l, g), ("rmean" | "rvar" | "dw" | "dbias" | "dgamma" | "dbeta", l, set),
    ("dimg" | "dplanes" | "dsvec", g). `masks` {(l, g): bool array}: the LeakyReLU branch taken in the backward (the device's
    a > 0); None: the chain's own. `scalars` (momentum, eps, slope) default to the case's as float32 values."""
    mom, eps, slope = scalars or (f32(c["momentum"]), f32(c["eps"]), f32(c["slope"]))
    G, B, C = c["G"], c["B"], c["C"]
    out = {}
    for g in range(G):
        p = t["params"][param_set(c, g)]
        a = t["img"][g]
        for l in range(1, LAYERS + 1):
            y, _ = conv(a, p["w"][l - 1], p["bias"][l - 1], svec=t["svec"][g] if l == 1 else None)
            mean, var, rstd, a = bn_fwd(y, p["gamma"][l - 1], p["beta"][l - 1], eps, slope)
            out["y", l, g], out["a", l, g], out["mean", l, g], out["rstd", l, g], out["var", l, g] = y, a, mean, rstd, var
    for s, p in enumerate(t["params"]):
        inst = [g for g in range(G) if param_set(c, g) == s]
        for l in range(1, LAYERS + 1):
            N = B * (64 >> l) ** 2
            out["rmean", l, s], out["rvar", l, s] = running(p["rmean"][l - 1], p["rvar"][l - 1],
                                                            [(out["mean", l, g], out["var", l, g]) for g in inst], N, mom)
            for k in ("dw", "dbias", "dgamma", "dbeta"):
                out[k, l, s] = 0.0
    for g in range(G):
        s = param_set(c, g)
        p = t["params"][s]
        da = np.asarray(t["dfeat"][g], dtype=np.float64)
        for l in range(LAYERS, 0, -1):
            mask = masks[l, g] if masks is not None else out["a", l, g] > 0
            r = bn_bwd(da, mask, out["y", l, g], out["mean", l, g], out["rstd", l, g], p["gamma"][l - 1], slope)
            out["dy", l, g] = r["dy"]
            a_in = t["img"][g] if l == 1 else out["a", l - 1, g]
            out["dw", l, s] = out["dw", l, s] + wgrad(r["dy"], a_in, svec=t["svec"][g] if l == 1 else None)[0]
            for k in ("dbias", "dgamma", "dbeta"):
                out[k, l, s] = out[k, l, s] + r[k]
            if l > 1:
                da = out["da", l - 1, g] = dgrad(r["dy"], p["w"][l - 1])[0]
            elif c["want"][g]:
                full = dgrad(r["dy"], p["w"][0])[0]
                out["dimg", g], out["dplanes", g] = full[:, :3], full[:, 3:]
                if c["n_state"]:
                    out["dsvec", g] = plane_sum(full[:, 3:])[0]
    return out


# ---- the stage-by-stage check ---------------------------------------------------------------------------------------------------------
def share(got, ref, A, K):
    """|got - ref| as a share of (K + 2) u A + u |ref| (tests/test_gpu_heads_stages._bounded); inf where the bound is 0 and the
    values differ."""
    err = np.abs(np.asarray(got, dtype=np.float64) - ref)
    bound = (np.asarray(K, dtype=np.float64) + 2) * U * A + U * np.abs(ref)
    return _ratio(err, bound)


def _ratio(err, bound):
    with np.errstate(divide="ignore", invalid="ignore"):
        return np.where(err == 0, 0.0, err / bound)


def stage_shares(c, t, got, emit, forward=True, backward=True, gemm=True):
    """Every stage of the buffers `got` (keys as `chain` returns them) against its float64 restatement on got's OWN upstream
    buffers; emit(label, shares, what) receives the element-wise share of the stage's bound. The bounds, with K the longest
    chain of additions the launch geometry gives and A the sum of the terms' magnitudes. A sum's bound is its worst case, which
    float32 arithmetic stays far below; an element-wise operation's worst case, u, is met, so those are allowed 4 u each: the
    quarter that tests/test_trunkref_host.py asks of float32 arithmetic is then the worst case itself. `gemm` False leaves
    out the three GEMM stages (their float64 references are the expensive part):

      conv      (K + 2) u A + u |y|, K = 16 Cin + 1 (every product and the bias)
      mean      the same form, K = ceil(N / nthr) (a thread's strided chain) + 6 (lane butterfly) + waves, A = sum |y| / N
      rstd      against (ssd / N + eps)^-1/2 with ssd = sum (y - mean)^2 about the buffers' OWN mean: relative error
                (K + 5) u / 2 . var / (var + eps) from ssd (each term three roundings, then the mean's chain) + 16 u (4 u
                for each of the division, eps, square root, reciprocal). The bound is relative to the variance, not to sum y^2.
      a         against bn_apply of the buffers' mean and rstd: 4 u per operation, 16 u T for the subtraction, two products and
                the addition (T = |(y - mean) rstd gamma| + |beta|), times the slope where z is safely negative, + 4 u |a|
      running   against `running` of the float64 statistics of the buffers' y: per update m times (the mean stage's bound | the
                ssd bound + delta^2 N / (N - 1), delta the mean stage's bound, because the kernel's ssd is about ITS mean) +
                12 u of the two terms (4 u per operation: 1 - m, the two products, the division, the addition: at most three
                on either term); an earlier instance's bound carried on times (1 - m)
      dbeta     (K + 3 + instances) u A1, A1 = sum |d|          (d = da or slope da: one rounding each)
      dgamma    (K + 6 + instances) u A2, A2 = sum |d x|        (x = (y - mean) rstd: two roundings, the product one)
      dy        |gamma rstd| (E1 / N + |x| E2 / N + 24 u (|d| + |m1| + |x m2|)) + 8 u |dy|, E1 / E2 the dbeta / dgamma bounds of
                one instance: the two means' errors, then 4 u per operation: at most six on each of d, m1, x m2 (slope, the two
                roundings of x, the division, the product, two subtractions), two on the result (gamma rstd, the last product)
      dbias     against the float64 sum of the buffers' OWN dy (what the kernel adds up; 0 but for the terms the formula leaves
                when mean is not exactly y's): (K + 2 + instances) u sum |dy|
      dw        K = 16 spw (x instances when one workgroup runs both) + KS + the partial tiles of the ordered reduction
      da / dimg / dplanes   K = 4 Cout
      dsvec     K = 16 + 6 + 4 (256 threads over 4096 pixels)"""
    mom, eps, slope = f32(c["momentum"]), f32(c["eps"]), f32(c["slope"])
    G, B, C = c["G"], c["B"], c["C"]
    geo = geometry(B, C, G if c["share"] else 1)
    stat = {}
    for g in range(G if forward else 0):
        p = t["params"][param_set(c, g)]
        for l in range(1, LAYERS + 1):
            what = f"{c['name']} layer {l} instance {g}"
            K, N = geo[l]["bn_K"], geo[l]["N"]
            a_in = t["img"][g] if l == 1 else got["a", l - 1, g]
            if gemm:
                y, A = conv(a_in, p["w"][l - 1], p["bias"][l - 1], svec=t["svec"][g] if l == 1 else None)
                emit("conv", share(got["y", l, g], y, A, 16 * C[l - 1] + 1), what)
            yd = np.asarray(got["y", l, g], dtype=np.float64)
            md, rd = (np.asarray(got[k, l, g], dtype=np.float64) for k in ("mean", "rstd"))
            mean = yd.mean(axis=(0, 2, 3))
            Am = np.abs(yd).mean(axis=(0, 2, 3))
            emit("mean", share(md, mean, Am, K), what)
            var_own = ((yd - md[None, :, None, None]) ** 2).mean(axis=(0, 2, 3))
            rstd = 1.0 / np.sqrt(var_own + eps)
            emit("rstd", _ratio(np.abs(rd - rstd), rstd * (0.5 * (K + 5) * U * var_own / (var_own + eps) + 16 * U)), what)
            a, z, T = bn_apply(yd, md, rd, p["gamma"][l - 1], p["beta"][l - 1], slope)
            emit("act", _ratio(np.abs(got["a", l, g] - a), np.where(z < -16 * U * T, slope, 1.0) * 16 * U * T + 4 * U * np.abs(a)), what)
            var = ((yd - mean[None, :, None, None]) ** 2).mean(axis=(0, 2, 3))
            dm = (K + 2) * U * Am + U * np.abs(mean)
            stat[l, g] = (mean, var, dm, ((K + 5) * U * var + dm * dm) * N / (N - 1))
    for s, p in enumerate(t["params"]):
        if ("rmean", 1, s) not in got or not forward:
            continue
        inst = [g for g in range(G) if param_set(c, g) == s]
        for l in range(1, LAYERS + 1):
            N = geo[l]["N"]
            rm, rv = np.asarray(p["rmean"][l - 1], dtype=np.float64), np.asarray(p["rvar"][l - 1], dtype=np.float64)
            bm, bv = 0.0, 0.0
            for g in inst:
                mean, var, dm, dv = stat[l, g]
                uv = var * N / (N - 1)
                bm = (1 - mom) * bm + mom * dm + 12 * U * (np.abs((1 - mom) * rm) + np.abs(mom * mean))
                bv = (1 - mom) * bv + mom * dv + 12 * U * (np.abs((1 - mom) * rv) + np.abs(mom * uv))
                rm, rv = running(rm, rv, [(mean, var)], N, mom)
            emit("running_mean", _ratio(np.abs(got["rmean", l, s] - rm), bm), f"{c['name']} layer {l} set {s}")
            emit("running_var", _ratio(np.abs(got["rvar", l, s] - rv), bv), f"{c['name']} layer {l} set {s}")
    if not backward:
        return
    for s, p in enumerate(t["params"]):
        inst = [g for g in range(G) if param_set(c, g) == s]
        ni = len(inst)
        for l in range(LAYERS, 0, -1):
            what = f"{c['name']} layer {l} set {s}"
            K, N = geo[l]["bn_K"], geo[l]["N"]
            tot = {k: 0.0 for k in ("dbeta", "dgamma", "A1", "A2", "dbias", "Ab", "dw", "Aw")}
            for g in inst:
                da = t["dfeat"][g] if l == LAYERS else got["da", l, g]
                r = bn_bwd(da, np.asarray(got["a", l, g]) > 0, got["y", l, g], got["mean", l, g], got["rstd", l, g],
                           p["gamma"][l - 1], slope)
                E1, E2 = (K + 4) * U * r["A1"], (K + 7) * U * r["A2"]
                cc = lambda v: v[None, :, None, None]  # noqa: E731
                bound = np.abs(cc(r["k0"])) * (cc(E1 / N) + np.abs(r["x"]) * cc(E2 / N) + 24 * U * (
                    np.abs(r["d"]) + np.abs(cc(r["m1"])) + np.abs(r["x"] * cc(r["m2"])))) + 8 * U * np.abs(r["dy"])
                emit("dy", _ratio(np.abs(got["dy", l, g] - r["dy"]), bound), f"{what} instance {g}")
                dyd = np.asarray(got["dy", l, g], dtype=np.float64)
                a_in = t["img"][g] if l == 1 else got["a", l - 1, g]
                dW, AW = wgrad(dyd, a_in, svec=t["svec"][g] if l == 1 else None) if gemm else (0.0, 0.0)
                for k, v in (("dbeta", r["dbeta"]), ("dgamma", r["dgamma"]), ("A1", r["A1"]), ("A2", r["A2"]),
                             ("dbias", dyd.sum(axis=(0, 2, 3))), ("Ab", np.abs(dyd).sum(axis=(0, 2, 3))), ("dw", dW), ("Aw", AW)):
                    tot[k] = tot[k] + v
                if gemm and (l > 1 or c["want"][g]):
                    full, Ad = dgrad(dyd, p["w"][l - 1])
                    Kd = 4 * C[l]
                    if l > 1:
                        emit("dgrad", share(got["da", l - 1, g], full, Ad, Kd), f"{what} instance {g}")
                    else:
                        emit("dgrad", share(got["dimg", g], full[:, :3], Ad[:, :3], Kd), f"{what} instance {g} dimg")
                        if c["n_state"]:
                            emit("dgrad", share(got["dplanes", g], full[:, 3:], Ad[:, 3:], Kd), f"{what} instance {g} planes")
                            ps, Ap = plane_sum(got["dplanes", g])
                            emit("plane_sum", share(got["dsvec", g], ps, Ap, 16 + 6 + 4), f"{what} instance {g}")
            emit("dbeta", share(got["dbeta", l, s], tot["dbeta"], tot["A1"], K + 1 + ni), what)
            emit("dgamma", share(got["dgamma", l, s], tot["dgamma"], tot["A2"], K + 4 + ni), what)
            emit("dbias", share(got["dbias", l, s], tot["dbias"], tot["Ab"], K + ni), what)
            if gemm:
                emit("wgrad", share(got["dw", l, s], tot["dw"], tot["Aw"], geo[l]["w_K"]), what)


# Chain-check bounds as fractions of each tensor's scale: 4x the largest fraction the float32 restatements of
# tests/test_trunkref_host.py reach against `chain` on the cases with B <= CHAIN_MAX_B (that test asserts the factor still
# holds), and never looser than the caps the module-path comparison of tests/test_gpu_trunk_train.py uses.
CHAIN_CAPS = dict(features=2e-5, running=1e-5, grad=2e-4, grad_input=2e-4)
CHAIN_HOST = dict(features=2.1e-6, running=3.1e-7, grad=3.2e-6, grad_input=1.1e-6)      # measured on the host, rounded up
CHAIN_FRAC = {k: min(CHAIN_CAPS[k], 4 * CHAIN_HOST[k]) for k in CHAIN_CAPS}
CHAIN_KEYS = {"features": ("a",), "running": ("rmean", "rvar"), "grad": ("dw", "dbias", "dgamma", "dbeta"),
              "grad_input": ("dimg", "dsvec")}


def chain_shares(c, t, got, emit):
    """Features, running statistics, every gradient and the input gradients of `got` against `chain` with the LeakyReLU masks
    taken from got's own activations, each error as a fraction of its tensor's largest |reference| value."""
    masks = {(l, g): np.asarray(got["a", l, g]) > 0 for l in range(1, LAYERS + 1) for g in range(c["G"])}
    ref = chain(c, t, masks=masks)
    for k, v in ref.items():
        if k not in got:
            continue
        for group, names in CHAIN_KEYS.items():
            if k[0] in names and (k[0] != "a" or k[1] == LAYERS):
                if k[0] == "dbias":                                     # exactly 0 in exact arithmetic: scaled by the weight gradient
                    scale = float(np.abs(ref["dw", k[1], k[2]]).max())
                else:
                    scale = float(np.abs(v).max())
                emit(group, _ratio(np.abs(np.asarray(got[k], dtype=np.float64) - v), scale), f"{c['name']} {k}")
