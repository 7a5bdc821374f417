"""The cases tests/test_gpu_policy_tail.py runs on the device and tests/test_tailref_host.py checks on the host: regressor
tables, batches, pre-activations, logits, noise, states and scalars, all from fixed seeds.

A discrete output (the sampled or arg-max id, the last-step flag) may not hang on fp32 rounding, so the generator re-draws an
image, deterministically, until `margins` holds for it; the host test asserts `margins` for every case, and the GPU tests then
skip nothing. Test infrastructure only."""
import math

import numpy as np

import _policyref as P
import _tailref as R

T_STEPS = 5.0

# (op, n, kind, lo, scale, bias); ops are the codes of include/adaisp.h, any will do for a table that is not the production one
F1 = [(6, 1, R.KIND_TANH, 0.0, 1.0, 0.0)]
F2 = [(9, 3, R.KIND_WB, -0.5, 1.0, 0.0), (12, 24, R.KIND_TANH_RANGE, 0.0, 2.0, 0.0)]
_F16 = [(0, 1, 0, -3.5, 7.0, 0.0), (1, 1, 1, -1.0986123, 2.1972246, 0.0), (2, 9, 0, -1.0, 2.0, 0.0), (4, 1, 2, 0.0, 1.0, 0.0),
        (6, 1, 3, 0.0, 1.0, 0.0), (9, 3, 4, -0.5, 1.0, 0.0), (12, 24, 0, 0.0, 1.0, 0.25), (1, 3, 1, -0.7, 1.4, -0.3),
        (7, 3, 2, 0.0, 1.0, 0.0), (5, 9, 3, 0.0, 1.0, 0.0), (10, 3, 0, 0.5, 1.5, 0.0), (9, 3, 4, -0.5, 1.0, 0.0),
        (2, 9, 0, -2.0, 4.0, 0.0), (8, 1, 2, 0.0, 1.0, 0.0), (1, 1, 1, -0.5, 1.0, 0.0)]
F16 = _F16 + [(5, 8, 0, 0.0, 1.0, 0.0)]              # 80 rows: 96 with the selector's 16, the last register round full
F16_97 = _F16 + [(5, 9, 0, 0.0, 1.0, 0.0)]           # 81 rows: 97, the row loop
F16_400 = [(5, 24, k % 4, -0.5 if k % 4 < 2 else 0.0, 1.0, 0.0) for k in range(16)]          # 384 rows: 400


def production():
    from adaptiveisp_amd.config import cfg
    return [make(cfg, predict=False).regressor_spec() for make in cfg.filters]


def tables():
    return {"prod10": production(), "f1": F1, "f2": F2, "f16": F16, "f16_97": F16_97, "f16_400": F16_400}


def scalars(specs, exploration, entropy_coef=0.037, usage=1.0, early=0.3, lam=0.01):
    """The float fields of the argument structs, as the float32 values they carry, and the op codes."""
    F = len(specs)
    f32 = lambda v: float(np.float32(v))  # noqa: E731
    return dict(one_minus_exploration=f32(1 - exploration), exploration_over_f=f32(exploration * 1.0 / F),
                entropy_coef=f32(entropy_coef), log_num_filters=f32(math.log(F)), test_steps=f32(T_STEPS),
                filter_usage_penalty=f32(usage), early_stop_penalty=f32(early), runtime_lambda=f32(lam),
                ops=[int(s[0]) for s in specs])


def margins(logits, u, step, sc, sample):
    """Per image: is every discrete output decided by more than fp32 rounding can move?
      sampling  min_k |cdf_exclusive_k - u| >= 1e-4 over k >= 1 (cdf_exclusive_0 is the exact 0 in any arithmetic: u > 0 takes
                it, the designed u = 0 does not);
      arg-max   the top-two pdf gap is >= 1e-4, or the two logits are bit-equal;
      last step | |step + 1 - T| - 1e-4 | >= 1e-5."""
    lg = np.asarray(logits, dtype=np.float64)
    import torch
    pdf = R._pdf(torch.as_tensor(lg), sc)[2].numpy()
    ok = np.abs(np.abs(np.asarray(step, dtype=np.float64) + 1.0 - sc["test_steps"]) - 1e-4) >= 1e-5
    if sample:
        cdf = R.cdf_exclusive(pdf)[:, 1:]
        if cdf.shape[1]:
            ok &= np.abs(cdf - np.asarray(u, dtype=np.float64)[:, None]).min(axis=1) >= 1e-4
    elif lg.shape[1] > 1:
        order = np.argsort(-pdf, axis=1, kind="stable")
        rows = np.arange(lg.shape[0])
        top, second = order[:, 0], order[:, 1]
        ok &= (pdf[rows, top] - pdf[rows, second] >= 1e-4) | (lg[rows, top] == lg[rows, second])
    return ok


U_SPECIAL = (0.0, 1e-7, 0.999999, 1.0)
STEPS = (T_STEPS - 1, T_STEPS - 1 + 5e-5, T_STEPS - 1 - 5e-5, T_STEPS - 1 + 1e-3, T_STEPS - 1 - 1e-3, 0.0, 1.0, 2.0)
SPREADS = (0.1, 1.0, 4.0, 10.0)
BIG = (None, 30.0, -30.0, 100.0, -100.0, None)


def _logits(rng, F, pattern, spread):
    lg = (rng.normal(size=F) * spread).astype(np.float32)
    lg = np.maximum(lg, lg.max() - np.float32(39.0))                        # |logit - max| <= 40 (the -120 below excepted)
    if F >= 3 and pattern == 1:
        lg[(int(np.argmax(lg)) + 1) % F] = lg.max() - np.float32(39.5)
    if F >= 2 and pattern == 3:                                             # two bit-equal maxima, the later one second
        k = int(np.argmax(lg))
        lg[(k + 1 + int(rng.integers(F - 1))) % F] = lg[k]
    if F >= 2 and pattern == 5:
        lg[F - 1] = np.float32(-120.0)
    return lg


def _image(seed, specs, pw, sc, sample, pattern):
    """One image's (x [F, pw], logits [F], u, state row [3 + F]); re-drawn until its margins hold."""
    F = len(specs)
    for attempt in range(200):
        rng = np.random.default_rng([*seed, attempt])
        x = rng.uniform(-4.0, 4.0, (F, pw)).astype(np.float32)
        for f, spec in enumerate(specs):                                    # saturating values in every kind
            big = BIG[(pattern + f) % len(BIG)]
            if big is not None:
                x[f, (pattern + f) % spec[1]] = big
        lg = _logits(rng, F, pattern % 7, SPREADS[pattern % len(SPREADS)])
        # a designed u that this image's pdf cannot take with a margin (0.999999 under a pdf that ends in 1e-37) gives way
        u = np.float32(U_SPECIAL[pattern % 8] if pattern % 8 < 4 and attempt < 20 else rng.random())
        st = np.zeros(3 + F, dtype=np.float32)
        st[:2] = rng.random(2)
        st[2] = STEPS[(pattern // 2) % len(STEPS)]
        st[3:] = rng.random(F) < 0.5
        if margins(lg[None], np.array([u]), st[2:3], sc, sample)[0]:
            return x, lg, u, st
    raise AssertionError(f"no draw of image {seed} passed the decision margins")


def _batch(tag, specs, B, idx, exploration, sample, forced_id, use_runtime, noise_stride, seed0):
    F, pw = len(specs), max(s[1] for s in specs)
    sc = scalars(specs, exploration)
    imgs = [_image((seed0, idx, b), specs, pw, sc, sample, idx + b) for b in range(B)]
    x, lg, u, st = (np.stack([im[k] for im in imgs]) for k in range(4))
    rng = np.random.default_rng([seed0, idx, 999])
    noise = rng.random((B, noise_stride)).astype(np.float32)               # the other columns must not be read
    noise[:, 0] = u
    return dict(name=f"{idx:02d}-{tag}-B{B}-e{exploration:g}-s{int(sample)}-f{forced_id}-r{int(use_runtime)}-ns{noise_stride}",
                seed=idx, specs=specs, F=F, pw=pw, B=B, x=x, logits=lg, u=u, noise=noise, noise_stride=noise_stride, states=st,
                scalars=sc, exploration=exploration, sample=int(sample), forced_id=forced_id,
                runtime=(0.5 + 10.0 * rng.random(F)).astype(np.float32) if use_runtime else None)


def _options(i, F):
    sample = i % 2 == 0
    forced = (-1, 0, F - 1)[(i // 2) % 3]
    exploration = (0.05, 0.0, 1.0)[i % 3]
    if exploration == 1.0 and not sample:
        exploration = 0.05          # every pdf is exploration / F then: an arg-max over equal values that are not equal logits
    return exploration, sample, forced, (i // 3) % 2 == 1, 1 + (i // 5) % 2


_CACHE = {}


def upstream(case):
    """(d_packed [B, pw], d_surrogate [B], d_penalty [B]) of a case's backward, float32."""
    rng = np.random.default_rng([31, case["seed"]])
    return tuple(rng.normal(size=s).astype(np.float32) for s in ((case["B"], case["pw"]), (case["B"],), (case["B"],)))


def tail_cases():
    """The cases of adaisp_policy_tail_fwd / _bwd: every table x B in {1, 3, 9, 70} x sampling on / off, the other options
    cycling, and designed ones after them."""
    if "tail" in _CACHE:
        return _CACHE["tail"]
    tb = tables()
    cases, i = [], 0
    for tag in ("prod10", "f1", "f2", "f16"):
        for B in (1, 3, 9, 70):
            for _ in range(2):
                cases.append(_batch(tag, tb[tag], B, i, *_options(i, len(tb[tag])), seed0=11))
                i += 1
    # designed: the arg-max over a tie and over the rest, unforced; the -120 logit forced with no exploration (pdf 1e-37: only
    # the surrogate's + 1e-10 keeps the log finite-sized); every u and step value sampled unforced at each exploration
    for tag in ("prod10", "f2", "f16"):
        F = len(tb[tag])
        cases.append(_batch(tag, tb[tag], 9, i, 0.05, False, -1, True, 1, seed0=12)); i += 1
        cases.append(_batch(tag, tb[tag], 9, i, 0.0, False, F - 1, False, 2, seed0=12)); i += 1
        cases.append(_batch(tag, tb[tag], 9, i, 0.0, True, F - 1, True, 1, seed0=12)); i += 1
        for e in (0.0, 0.05, 1.0):
            cases.append(_batch(tag, tb[tag], 9, i, e, True, -1, e != 0.05, 2, seed0=12)); i += 1
    _CACHE["tail"] = cases
    return cases


# (table, hid, B): hid 8 .. 256 with at most 96 rows is k_finish's register path; hid > 256 or more rows its loop
FINISH_SHAPES = [("prod10", 128, 3), ("prod10", 8, 1), ("f1", 72, 9), ("f2", 256, 3), ("f16", 128, 3), ("f16_97", 128, 1),
                 ("f16_400", 72, 2), ("prod10", 264, 3), ("f2", 320, 70), ("f16", 256, 9)]


def finish_cases():
    """The cases of adaisp_policy_finish: hidden, both weight sets and biases on power-of-two lattices (hidden step 2^-2 within
    1, head weights step 2^-4 within 1, selector weights step 2^-6 within 2^-4, biases step 2^-6 within 1), so every
    pre-activation is exact in float32 in any summation order; x and logits are those dot products, taken in float64."""
    if "finish" in _CACHE:
        return _CACHE["finish"]
    tb = tables()
    cases = []
    for i, (tag, hid, B) in enumerate(FINISH_SHAPES):
        specs = tb[tag]
        F, pw = len(specs), max(s[1] for s in specs)
        exploration, sample, forced, use_runtime, noise_stride = _options(i + 1, F)
        sc = scalars(specs, exploration)
        rows_f = np.array([f for f, s in enumerate(specs) for _ in range(s[1])], dtype=np.int32)
        rows_s = np.array([k for s in specs for k in range(s[1])], dtype=np.int32)
        wrng = np.random.default_rng([21, i])
        w_filter, b_filter = P.lattice(wrng, (len(rows_f), hid), 2.0 ** -4, 1.0), P.lattice(wrng, (len(rows_f),), 2.0 ** -6, 1.0)
        w_sel, b_sel = P.lattice(wrng, (F, hid), 2.0 ** -6, 2.0 ** -4), P.lattice(wrng, (F,), 2.0 ** -6, 1.0)
        hidden, us, sts = [], [], []
        for b in range(B):
            pattern = i + b
            for attempt in range(200):
                rng = np.random.default_rng([22, i, b, attempt])
                h = P.lattice(rng, (F + 1, hid), 2.0 ** -2, 1.0)
                lg = h[F].astype(np.float64) @ w_sel.astype(np.float64).T + b_sel
                u = np.float32(U_SPECIAL[pattern % 8] if pattern % 8 < 4 and attempt < 20 else rng.random())
                st = np.zeros(3 + F, dtype=np.float32)
                st[:2] = rng.random(2)
                st[2] = STEPS[(pattern // 2) % len(STEPS)]
                st[3:] = rng.random(F) < 0.5
                if margins(lg[None], np.array([u]), st[2:3], sc, sample)[0]:
                    break
            else:
                raise AssertionError(f"no draw of finish image {(i, b)} passed the decision margins")
            hidden.append(h); us.append(u); sts.append(st)
        hidden, u, st = np.stack(hidden), np.array(us, dtype=np.float32), np.stack(sts)
        h64 = hidden.astype(np.float64)
        x = np.zeros((B, F, pw))
        x[:, rows_f, rows_s] = np.einsum("brh,rh->br", h64[:, rows_f], w_filter.astype(np.float64)) + b_filter
        logits = h64[:, F] @ w_sel.astype(np.float64).T + b_sel
        assert np.array_equal(x.astype(np.float32), x) and np.array_equal(logits.astype(np.float32), logits)
        rng = np.random.default_rng([23, i])
        noise = rng.random((B, noise_stride)).astype(np.float32)
        noise[:, 0] = u
        cases.append(dict(name=f"fin{i}-{tag}-hid{hid}-B{B}-rows{len(rows_f) + F}-e{exploration:g}-s{int(sample)}-f{forced}", seed=1000 + i, specs=specs,
                          F=F, pw=pw, B=B, hid=hid, hidden=hidden, w_filter=w_filter, b_filter=b_filter, w_sel=w_sel, b_sel=b_sel,
                          row_filter=rows_f, row_slot=rows_s, x=x.astype(np.float32), logits=logits.astype(np.float32), u=u,
                          noise=noise, noise_stride=noise_stride, states=st, scalars=sc, exploration=exploration,
                          sample=int(sample), forced_id=forced,
                          runtime=(0.5 + 10.0 * rng.random(F)).astype(np.float32) if use_runtime else None))
    _CACHE["finish"] = cases
    return cases
