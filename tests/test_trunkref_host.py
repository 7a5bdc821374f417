"""tests/_trunkref.py is the float64 reference that tests/test_gpu_trunk_stages.py holds the training-mode trunk kernels to.
Here, on the host:

  pin       `chain` with its own masks is nets.FeatureExtractor in .train() under float64 autograd: features, every parameter
            gradient, the input and state-vector gradients, the running statistics and num_batches_tracked, to 1e-11 of scale;
  headroom  a float32 numpy restatement of every stage, in two summation orders, uses at most a quarter of every stage bound on
            every case the device runs. One order is the kernels' own: a thread's strided chain, then the lane butterfly and the
            waves in order; slices of channels / pixel steps that meet in slice order. The other is plain sequential summation
            where the bound counts every term (conv, data gradient); where the bound counts the kernel's own chain (the
            statistics, their backward sums, the weight gradient, the plane sum: a sequential sum over N = 525 312 values
            is not what such a bound describes) it is the same reduction over the REVERSED element order, i.e. other elements per
            thread and another order inside every chain. The statistics stages are restated in full; the three GEMM stages run
            in full through a float32 matmul (a third, blocked order) and in the two exact orders on a subset of their outputs
            (first / last images and channels), so B = 513 stays at seconds;
  mutants   each of eleven deliberate errors in that restatement breaks a stage bound on a listed case;
  coverage  the case list reaches the launch geometries the device test's docstring claims, and that docstring's table is
            _trunkref.geometry_table()."""
import numpy as np
import pytest
import torch

import _policyref as P
import _trunkref as R

F = np.float32
L4 = R.LAYERS


# ---- pin -----------------------------------------------------------------------------------------------------------------------
def _module(c, p):
    from adaptiveisp_amd.nets import FeatureExtractor
    m = FeatureExtractor(shape=(c["C"][0], 64, 64), mid_channels=c["C"][1], output_dim=16 * c["C"][4], dropout_prob=None).double()
    with torch.no_grad():
        for l in range(L4):
            conv, bn = m.layers[3 * l], m.layers[3 * l + 1]
            assert tuple(conv.weight.shape) == p["w"][l].shape
            for dst, k in ((conv.weight, "w"), (conv.bias, "bias"), (bn.weight, "gamma"), (bn.bias, "beta"),
                           (bn.running_mean, "rmean"), (bn.running_var, "rvar")):
                dst.copy_(torch.from_numpy(p[k][l].astype(np.float64)))
    return m.train()


PIN = [R._case("pin-b1", 1, 13, R.PROD, G=1, want=(0,)), R._case("pin-b3", 3, 13, R.PROD, G=2, special="zero"),
       R._case("pin-b8", 8, 13, R.PROD, G=1, want=(0,)),
       R._case("pin-two-calls", 3, 13, R.PROD, G=2, share=True, n_in=2, want=(0, 1), special="zero"),
       R._case("pin-no-state", 3, 0, R.PROD, G=1, want=(0,))]


@pytest.mark.parametrize("c", PIN, ids=[c["name"] for c in PIN])
def test_chain_is_the_module_under_float64_autograd(c):
    t = R.inputs(c, seed=3)
    ref = R.chain(c, t, scalars=(0.1, 1e-5, 0.2))
    mods = [_module(c, p) for p in t["params"]]

    def agree(got, want, what):
        want = want.detach().numpy() if hasattr(want, "detach") else np.asarray(want)
        scale = max(float(np.abs(want).max()), 1e-30)
        assert np.abs(np.asarray(got).reshape(want.shape) - want).max() <= 1e-11 * scale, what

    leaves, feats = [], []
    for g in range(c["G"]):
        img = torch.from_numpy(t["img"][g].astype(np.float64)).requires_grad_(True)
        sv = torch.from_numpy(t["svec"][g].astype(np.float64)).requires_grad_(True) if c["n_state"] else None
        x = img if sv is None else torch.cat([img, sv[:, :, None, None].expand(-1, -1, 64, 64)], dim=1)
        feats.append(mods[R.param_set(c, g)](x))
        leaves.append((img, sv))
    loss = sum((f * torch.from_numpy(t["dfeat"][g].astype(np.float64)).reshape(f.shape)).sum() for g, f in enumerate(feats))
    loss.backward()
    for g in range(c["G"]):
        agree(ref["a", L4, g], feats[g], f"features {g}")
        if c["want"][g]:
            agree(ref["dimg", g], leaves[g][0].grad, f"dimg {g}")
            if c["n_state"]:
                agree(ref["dsvec", g], leaves[g][1].grad, f"dsvec {g}")
    for s, m in enumerate(mods):
        calls = sum(1 for g in range(c["G"]) if R.param_set(c, g) == s)
        for l in range(L4):
            conv, bn = m.layers[3 * l], m.layers[3 * l + 1]
            assert int(bn.num_batches_tracked) == calls                                  # one update per instance, in order
            agree(ref["rmean", l + 1, s], bn.running_mean, f"running_mean {l}")
            agree(ref["rvar", l + 1, s], bn.running_var, f"running_var {l}")
            agree(ref["dw", l + 1, s], conv.weight.grad, f"dw {l}")
            agree(ref["dgamma", l + 1, s], bn.weight.grad, f"dgamma {l}")
            agree(ref["dbeta", l + 1, s], bn.bias.grad, f"dbeta {l}")
            # the conv bias in front of batch statistics: 0 in exact arithmetic on both sides, held to the weight gradient's scale
            wscale = float(conv.weight.grad.abs().max())
            assert np.abs(ref["dbias", l + 1, s]).max() <= 1e-11 * wscale and float(conv.bias.grad.abs().max()) <= 1e-11 * wscale
    if c["special"]:                                                                     # z = 0 exactly: torch's x > 0 rule
        assert not ref["a", 2, 0][:, 7].any()      # (the 1e3 offset channel is left out here: float64 itself loses 4 digits on it)


def test_plan_totals_and_offsets():
    p = R.plan(8, (16, 32, 64, 128, 256), 2)
    n = [8 * c * h * h for c, h in zip((32, 64, 128, 256), (32, 16, 8, 4))]
    assert p["ws_per_g"] == 2 * sum(n[:3]) + n[3] + 2 * (32 + 64 + 128 + 256)
    assert p["scr_per_g"] == 2 * sum(n[:3]) + n[3] + 8 * 16 * 4096 and p["wpart"] == 2 * p["scr_per_g"]
    assert p["y"][1] == 0 and p["a"][1] == n[0] and p["mean"][1] == 2 * n[0] and p["y"][2] == 2 * n[0] + 64
    assert p["wpart_size"] == 8 * 2 * 32 * 16 * 16                                       # layer 1: 512 steps in 8 chunks


# ---- the float32 restatement ---------------------------------------------------------------------------------------------------
def _seq(v):
    """Sequential float32 sum over the last axis."""
    return np.cumsum(v, axis=-1, dtype=F)[..., -1]


def _block_sum(v, nthr):
    """block_sum of isp_policy_math.h over rows [R, N] in element order: thread tid adds elements tid, tid + nthr, ..., the 64
    lanes of a wave meet in an xor butterfly, the waves are added in index order."""
    Rr, N = v.shape
    trips = -(-N // nthr)
    pad = np.zeros((Rr, trips * nthr), dtype=F)
    pad[:, :N] = v
    s = _seq(pad.reshape(Rr, trips, nthr).transpose(0, 2, 1)).reshape(Rr, nthr // 64, 64)
    lanes = np.arange(64)
    for off in (32, 16, 8, 4, 2, 1):
        s = s + s[:, :, lanes ^ off]
    return _seq(s[:, :, 0])


def _sum(v, order, nthr):
    """block_sum in the kernel's element order, or ("other") in the reversed one: another assignment of elements to threads and
    another order inside every chain, with the chain lengths the bound counts."""
    return _block_sum(v if order == "kernel" else v[:, ::-1], nthr)


def _rows(y):
    return np.ascontiguousarray(y.transpose(1, 0, 2, 3)).reshape(y.shape[1], -1)


def _col(v):
    return v[None, :, None, None]


def _patches32(x, Ho, const_from=None):
    p = P._patches(x, Ho)
    if const_from is not None:                                                           # mutant: the planes constant in the padding too
        planes = np.broadcast_to(x[:, const_from:, :1, :1], x[:, const_from:].shape[:2] + (2 * Ho + 2, 2 * Ho + 2))
        xp = np.concatenate([np.pad(x[:, :const_from], ((0, 0), (0, 0), (1, 1), (1, 1))), planes], axis=1)
        taps = [xp[:, :, kh:kh + 2 * Ho:2, kw:kw + 2 * Ho:2] for kh in range(4) for kw in range(4)]
        p = np.stack(taps, axis=2).reshape(x.shape[0], -1, Ho * Ho)
    return p.astype(F)


def _input32(t, g, l, got):
    return R._full_input(t["img"][g], t["svec"][g]).astype(F) if l == 1 else got["a", l - 1, g]


def run32(c, t, order, mutant=None):
    """The whole pass in float32 numpy -> buffers keyed like _trunkref.chain. Statistics sums in `order` ("kernel" | "other");
    the GEMM stages through a float32 matmul."""
    mom, eps, slope = F(c["momentum"]), F(c["eps"]), F(c["slope"])
    G, B, C, S = c["G"], c["B"], c["C"], c["n_state"]
    geo = R.geometry(B, C, G if c["share"] else 1)
    got, ssd = {}, {}
    for l in range(1, L4 + 1):
        N, nthr, Ho = geo[l]["N"], geo[l]["nthr"], 64 >> l
        for g in range(G):
            p = t["params"][R.param_set(c, g)]
            x = _input32(t, g, l, got)
            w = p["w"][l - 1].reshape(C[l], -1).copy()
            if mutant == "masked channels past Cin contributing":                       # the padded slots re-read channel Cin - 1
                w.reshape(C[l], C[l - 1], 16)[:, -1] *= F(1 + geo[l]["cpad"])
            y = np.concatenate([np.matmul(w[None], _patches32(x[b0:b0 + R.CHUNK], Ho, 3 if mutant == "state planes not zero-padded"
                                                               and l == 1 and S else None)) for b0 in range(0, B, R.CHUNK)])
            y = (y + p["bias"][l - 1][None, :, None]).reshape(B, C[l], Ho, Ho)
            v = _rows(y)
            mean = _sum(v, order, nthr) / F(N)
            if mutant == "one-pass variance":
                sd = _sum(v * v, order, nthr) - F(N) * mean * mean
            else:
                d = v - mean[:, None]
                sd = _sum(d * d, order, nthr)
            got["y", l, g], got["mean", l, g], got["rstd", l, g], ssd[l, g] = y, mean, F(1) / np.sqrt(sd / F(N) + eps), sd
        for g in range(G):
            p = t["params"][R.param_set(c, g)]
            o = G - 1 - g if mutant == "statistics swapped between the instances" else g
            z = ((got["y", l, g] - _col(got["mean", l, o])) * _col(got["rstd", l, o])) * _col(p["gamma"][l - 1]) + _col(p["beta"][l - 1])
            if mutant == "slope on the wrong branch":
                got["a", l, g] = np.where(z > 0, z * slope, z)
            else:
                got["a", l, g] = np.where(z > 0, z, z * slope)
        for s, p in enumerate(t["params"]):
            inst = [g for g in range(G) if R.param_set(c, g) == s]
            rm, rv = p["rmean"][l - 1], p["rvar"][l - 1]
            for g in (inst[-1:] if mutant == "momentum applied once for two instances" else inst):
                rm = (F(1) - mom) * rm + mom * got["mean", l, g]
                rv = (F(1) - mom) * rv + mom * (ssd[l, g] / F(N if mutant == "biased running variance" else N - 1))
            got["rmean", l, s], got["rvar", l, s] = rm, rv
    for l in range(L4, 0, -1):
        N, nthr, Ho = geo[l]["N"], geo[l]["nthr"], 64 >> l
        for s, p in enumerate(t["params"]):
            inst = [g for g in range(G) if R.param_set(c, g) == s]
            tg = tb = tbias = dW = None
            for g in inst:
                da = t["dfeat"][g] if l == L4 else got["da", l, g]
                a = got["a", l, g]
                d = np.where(a >= 0 if mutant == "mask a >= 0" else a > 0, da, da * slope)
                x = (got["y", l, g] - _col(got["mean", l, g])) * _col(got["rstd", l, g])
                s1, s2 = _sum(_rows(d), order, nthr), _sum(_rows(d * x), order, nthr)
                k0 = p["gamma"][l - 1] * got["rstd", l, g]
                dy = (d - _col(s1 / F(N)) - x * _col(s2 / F(N))) * _col(k0)
                s3 = _sum(_rows(dy), order, nthr)
                got["dy", l, g] = dy
                first = tg is None
                tg = s2 if first or mutant == "dgamma not summed over the instances" else tg + s2
                tb, tbias = (s1, s3) if first else (tb + s1, tbias + s3)
                dyw = dy.reshape(B, C[l], -1)
                if mutant == "last pixel step of a chunk dropped":
                    flat = dyw.transpose(1, 0, 2).reshape(C[l], geo[l]["PS"], -1).copy()
                    flat[:, :, -16:] = 0
                    dyw = flat.reshape(C[l], B, -1).transpose(1, 0, 2)
                xin = _input32(t, g, l, got)
                part = sum(np.matmul(dyw[b0:b0 + R.CHUNK], _patches32(xin[b0:b0 + R.CHUNK], Ho).transpose(0, 2, 1)).sum(axis=0, dtype=F)
                           for b0 in range(0, B, R.CHUNK))
                dW = part if first else dW + part
                if l > 1 or c["want"][g]:
                    full = np.zeros((B, C[l - 1], 2 * Ho, 2 * Ho), dtype=F)
                    for ry in range(2):
                        for rx in range(2):
                            edge = 2 if mutant == "one border tap unmasked" and (ry, rx) == (0, 0) else None
                            D, Wc = R.dgrad_terms(dy, p["w"][l - 1], ry, rx, dtype=F, edge=edge)
                            full[:, :, ry::2, rx::2] = np.matmul(Wc[None], D).reshape(B, -1, Ho, Ho)
                    if l > 1:
                        got["da", l - 1, g] = full
                    else:
                        got["dimg", g] = full[:, :3]
                        if S:
                            got["dplanes", g] = full[:, 3:]
                            got["dsvec", g] = _sum(full[:, 3:].reshape(B * S, -1), order, 256).reshape(B, S)
            got["dgamma", l, s], got["dbeta", l, s], got["dbias", l, s] = tg, tb, tbias
            got["dw", l, s] = dW.reshape(p["w"][l - 1].shape)
    return got


def _sliced(terms, slices, order):
    """Float32 sum over the last axis: "other" sequentially in the axis' order; "kernel": each index list of `slices` is one wave's chain, the
    waves' totals are added in slice order (meet_in_lds)."""
    if order == "other":
        return _seq(terms)
    tot = None
    for idx in slices:
        if len(idx):
            part = _seq(terms[..., idx])
            tot = part if tot is None else tot + part
    return tot


def _pick(n, k):
    return sorted(set(range(min(k, n))) | set(range(max(0, n - k), n)))


def gemm_shares(c, t, got, order, emit):
    """k_tconv_fwd, k_twgrad (+ k_twgrad_reduce) and k_tdgrad in float32 in the exact `order`, on a subset of their outputs (the
    first and last images / channels), against the same sums in float64, as shares of the device test's bounds."""
    G, B, C = c["G"], c["B"], c["C"]
    geo = R.geometry(B, C, G if c["share"] else 1)
    imgs = _pick(B, 1)
    for l in range(1, L4 + 1):
        Cin, Cout, Ho, q = C[l - 1], C[l], 64 >> l, geo[l]
        co = _pick(Cout, 8)
        # conv: a wave's chain runs over its channels, per channel kw outer (the four MFMAs), kh inner (an MFMA's k)
        cslices = [[ci * 16 + kh * 4 + kw for ci in range(ks * q["ccpw"], min(Cin, (ks + 1) * q["ccpw"])) for kw in range(4) for kh in range(4)]
                   for ks in range(q["cKS"])]
        # weight gradient: pixel 16 st + 4 kq + j of step st enters MFMA j as k = kq
        lane = np.array([4 * kq + j for j in range(4) for kq in range(4)])
        n_of = lambda a, b: (16 * np.arange(a, b)[:, None] + lane[None, :]).ravel()  # noqa: E731
        per = q["N"] // 16 // q["PS"]
        # data gradient: slices of cpw output channels, (co, tap) in order
        dslices = [list(range(ks * q["dcpw"] * 4, (ks + 1) * q["dcpw"] * 4)) for ks in range(q["dKS"])]
        for s, p in enumerate(t["params"]):
            inst = [g for g in range(G) if R.param_set(c, g) == s]
            w = p["w"][l - 1]
            big = q["N"] > 1 << 16                                                       # (fewer outputs where each has many terms)
            ci_sub = _pick(Cin, 1 if big else 2)
            ksub = [ci * 16 + k for ci in ci_sub for k in range(16)]
            co2 = [Cout - 1] if big else _pick(Cout, 1)
            wt = []                                                                      # per instance [co2, ksub, N] float32 terms
            for g in inst:
                x = _input32(t, g, l, got)
                pt = _patches32(x[imgs], Ho)                                             # [b, K, P]
                terms = w.reshape(Cout, -1)[co][None, :, None, :] * pt.transpose(0, 2, 1)[:, None]      # [b, co, P, K]
                t64 = terms.astype(np.float64)
                bias = p["bias"][l - 1][co][None, :, None]
                emit("conv", R.share(_sliced(terms, cslices, order) + bias, t64.sum(-1) + bias, np.abs(t64).sum(-1) + np.abs(bias),
                                     16 * Cin + 1), f"{c['name']} L{l} {order}")
                dy = got["dy", l, g]
                pk = np.concatenate([_patches32(x[b0:b0 + R.CHUNK], Ho)[:, ksub] for b0 in range(0, B, R.CHUNK)])     # [B, ksub, P]
                wt.append(dy[:, co2].transpose(1, 0, 2, 3).reshape(len(co2), 1, -1) * pk.transpose(1, 0, 2).reshape(1, len(ksub), -1))
                if l > 1 or c["want"][g]:
                    cin_sub = _pick(Cin, 4)
                    for ry in range(2):
                        for rx in range(2):
                            D, Wc = R.dgrad_terms(dy[imgs], w, ry, rx, dtype=F)
                            terms = Wc[cin_sub][None, :, None, :] * D.transpose(0, 2, 1)[:, None]               # [b, ci, P, K]
                            t64 = terms.astype(np.float64)
                            emit("dgrad", R.share(_sliced(terms, dslices, order), t64.sum(-1), np.abs(t64).sum(-1), 4 * Cout),
                                 f"{c['name']} L{l} {order}")
            t64 = sum(v.astype(np.float64).sum(-1) for v in wt)
            A = sum(np.abs(v.astype(np.float64)).sum(-1) for v in wt)
            if order == "other":                                                         # the same launch over the reversed pixel order
                wt = [v[..., ::-1] for v in reversed(wt)]
            if q["PS"] == 1:                                                           # a wave runs its steps of every instance
                waves = [np.concatenate([v[..., n_of(ks * q["spw"], (ks + 1) * q["spw"])] for v in wt], axis=-1)
                         for ks in range(q["wKS"])]
                dw = _seq(np.stack([_seq(v) for v in waves], axis=-1))
            else:                                                                        # partial tiles, added in (instance, chunk) order
                parts = []
                for v in wt:
                    for ch in range(q["PS"]):
                        waves = [_seq(v[..., n_of(ch * per + ks * q["spw"], ch * per + (ks + 1) * q["spw"])])
                                 for ks in range(q["wKS"])]
                        parts.append(_seq(np.stack(waves, axis=-1)))
                dw = _seq(np.stack(parts, axis=-1))
            emit("wgrad", R.share(dw, t64, A, q["w_K"]), f"{c['name']} L{l} {order}")


MUTANTS = ["one-pass variance", "biased running variance", "momentum applied once for two instances", "mask a >= 0",
           "slope on the wrong branch", "last pixel step of a chunk dropped", "one border tap unmasked",
           "state planes not zero-padded", "masked channels past Cin contributing", "statistics swapped between the instances",
           "dgamma not summed over the instances"]


def _collect(into):
    def emit(label, shares, what):
        v = float(np.max(shares))
        if not v <= into.get(label, (-1.0, ""))[0]:
            into[label] = (v, what)
    return emit


_INPUTS = {}


def _inputs(i):
    if i not in _INPUTS:
        _INPUTS.clear()                                                                  # (one case's inputs at a time)
        _INPUTS[i] = R.inputs(R.CASES[i])
    return _INPUTS[i]


@pytest.mark.parametrize("i", range(len(R.CASES)), ids=[c["name"] for c in R.CASES])
def test_float32_restatements_use_a_quarter_of_each_bound(i):
    c, t = R.CASES[i], _inputs(i)
    worst, chain = {}, {}
    for order in ("kernel", "other"):
        got = run32(c, t, order)
        keep = _collect(worst)
        # (the matmul's weight gradient is one chain over all pixels: not what a bound on the kernel's chain describes)
        R.stage_shares(c, t, got, lambda label, sh, what: None if label == "wgrad" else keep(label, sh, what), gemm=order == "kernel")
        gemm_shares(c, t, got, order, keep)
        if c["B"] <= R.CHAIN_MAX_B:
            R.chain_shares(c, t, got, _collect(chain))
    print({k: (round(v, 4), w) for k, (v, w) in worst.items()})
    print({k: (float(f"{v:.3g}"), w) for k, (v, w) in chain.items()})
    assert set(worst) >= {"conv", "mean", "rstd", "act", "dy", "dbeta", "dgamma", "dbias", "wgrad", "dgrad"}
    bad = {k: v for k, v in worst.items() if not v[0] <= 0.25}
    assert not bad, f"float32 arithmetic uses more than 0.25 of the bound: {bad}"
    # the chain check's fractions are still at least 4x what float32 arithmetic reaches here, and within the call-site caps
    for k, (v, w) in chain.items():
        assert v <= R.CHAIN_FRAC[k] / 4 and R.CHAIN_FRAC[k] <= R.CHAIN_CAPS[k], (k, v, w)


@pytest.mark.parametrize("mutant", MUTANTS)
def test_mutant_breaks_a_stage_bound(mutant):
    for i, c in enumerate(R.CASES):
        if c["B"] > 129:                                                                 # (the offset channel is first met at B = 129)
            break
        worst = {}
        R.stage_shares(c, _inputs(i), run32(c, _inputs(i), "kernel", mutant), _collect(worst))
        hit = {k: v for k, v in worst.items() if not v[0] <= 1.0}
        if hit:
            print(f"{mutant}: {hit}")
            return
    raise AssertionError(f"'{mutant}' passes every stage bound on every case up to B = 129")


# ---- coverage ------------------------------------------------------------------------------------------------------------------
def test_case_list_reaches_the_geometries_the_device_test_claims():
    geos = [(c, R.geometry(c["B"], c["C"], c["G"] if c["share"] else 1)) for c in R.CASES]
    names = [c["name"] for c in R.CASES]
    assert len(set(names)) == len(names) == 13
    for l in range(1, L4 + 1):
        assert any(g[l]["bn"] == "STREAM" for _, g in geos), f"no streaming BatchNorm at layer {l}"
    assert any(g[4]["nthr"] == 64 and g[4]["N"] == 16 for _, g in geos)
    assert {g[l]["U"] for _, g in geos for l in g} == {1, 2, 4}
    assert {g[l]["wKS"] for _, g in geos for l in g} >= {1, 9, 11, 12, 16}
    assert any(g[l]["wKS"] == 1 and g[l]["spw"] == 17 for _, g in geos for l in g)
    assert any(g[l]["spw"] == 7 for _, g in geos for l in g) and any(g[l]["spw"] == 5 for _, g in geos for l in g)
    assert any(c["share"] and g[l]["PS"] > 1 for c, g in geos for l in g)
    assert any(g[l]["cpad"] > 0 and g[l]["cmasked"] >= 1 for _, g in geos for l in g)
    assert any(g[l]["cKS"] == 16 and g[l]["ccpw"] == 16 and g[l]["cmasked"] == 4 for _, g in geos for l in g)
    assert any(g[l]["dKS"] == 12 for _, g in geos for l in g) and any(g[l]["dcpw"] == 24 for _, g in geos for l in g)
    assert any(c["n_state"] == 0 and g[1]["cKS"] == 1 and g[1]["cpad"] == 5 for c, g in geos)
    assert sum(c["special"] is True for c in R.CASES) >= 2 and sum(bool(c["special"]) for c in R.CASES) >= 4 and any(c["null_running"] for c in R.CASES)
    assert any((c["momentum"], c["eps"], c["slope"]) == (0.3, 1e-3, 0.01) for c in R.CASES)
    assert any(c["want"] == (False, True) for c in R.CASES) and any(c["want"] == (True, True) for c in R.CASES)


def test_device_test_docstring_lists_the_geometry():
    import os
    src = open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "test_gpu_trunk_stages.py")).read()
    assert R.geometry_table() in src.split('"""')[1]
