"""Float64 restatements of the policy's finish / tail arithmetic (csrc/isp_policy_math.h: regress, regress_grad, select_tail, as
run by k_finish, k_policy_tail_fwd and k_policy_tail_bwd) and of the six training heads kernels (csrc/isp_heads_train.hip), host
only. tests/test_tailref_host.py pins them to the project's ATen statements in double precision before the device is compared
with them (tests/test_gpu_policy_tail.py, tests/test_gpu_heads_stages.py).

Every tail function returns its value and, per element, a magnitude S; a device result must satisfy
    |got - ref| <= CAP * S + 1e-30.
CAP = 1e-5 is the project's figure for fp32 arithmetic that goes through device transcendentals (RTOL of test_gpu_parity.py,
PARAM_CAP of the gradient sweep) — a cap the project sets, not a measurement of the device. The 1e-30 term covers results
below the fp32 normal range, where device functions may flush. S is built by first-order error propagation: sums and
differences add their S, a product scales S by the other factor's magnitude, f(v) gets |f| + |f'(v)| S(v). With
S_v = 2 (|scale| + |lo|) for the tanh_range value v that gives the forms written next to each function below.

The heads functions return the value and A = sum |products| + |bias|, the magnitude the summation bound
(K + 2) u A + u |ref| of the device tests scales with (u = 2^-24), as tests/_policyref.py does. Test infrastructure only."""
import numpy as np
import torch

CAP = 1e-5
TINY = 1e-30
KIND_TANH_RANGE, KIND_EXP_TANH_RANGE, KIND_SIGMOID, KIND_TANH, KIND_WB = range(5)   # enum adaisp_regressor_kind
OP_ZERO = -1                                                                         # ADAISP_OP_ZERO
LUM_W = (0.27, 0.67, 0.06)
SCALAR_FIELDS = ("one_minus_exploration", "exploration_over_f", "entropy_coef", "log_num_filters", "test_steps",
                 "filter_usage_penalty", "early_stop_penalty", "runtime_lambda")


def normalised(got, ref, S):
    """(got / s, ref / s) with s = S + 1e-30 / CAP: |got - ref| <= CAP * S + 1e-30 is then `close(..., rtol=0, atol=CAP)`."""
    s = np.asarray(S, dtype=np.float64) + TINY / CAP
    return np.asarray(got, dtype=np.float64) / s, np.asarray(ref, dtype=np.float64) / s


def _t(a):
    return a if isinstance(a, torch.Tensor) else torch.as_tensor(np.asarray(a, dtype=np.float64))


def _f32(v):
    return float(np.float32(v))


def spec_consts(spec):
    """(n, kind, lo, scale, bias, S_v) of an (op, n, kind, lo, scale, bias) entry; lo, scale and bias as the float32 values the
    adaisp_regressor struct carries."""
    _, n, kind, lo, scale, bias = spec
    lo, scale, bias = _f32(lo), _f32(scale), _f32(bias)
    return int(n), int(kind), lo, scale, bias, 2.0 * (abs(scale) + abs(lo))


def regress(spec, row):
    """The n regressed parameters of one filter from its head's pre-activations row [..., >= n] (torch double; differentiable).
    Returns (out [..., n], S [..., n] numpy): TANH_RANGE S_v; EXP_TANH_RANGE e^v (1 + S_v); SIGMOID, TANH 1; WB 2 out (1 + S_v)."""
    n, kind, lo, scale, bias, Sv = spec_consts(spec)
    x = _t(row)[..., :n]
    if kind == KIND_SIGMOID:
        out = 1.0 / (1.0 + torch.exp(-x))
        return out, np.ones(out.shape)
    if kind == KIND_TANH:
        out = torch.tanh(x)
        return out, np.ones(out.shape)
    if kind == KIND_WB:
        assert n == 3
        x = x * torch.tensor([0.0, 1.0, 1.0], dtype=torch.float64)           # the R gain is pinned
    v = (torch.tanh(x + bias) * 0.5 + 0.5) * scale + lo
    if kind == KIND_TANH_RANGE:
        return v, np.full(v.shape, Sv)
    g = torch.exp(v)
    if kind == KIND_EXP_TANH_RANGE:
        return g, g.detach().numpy() * (1.0 + Sv)
    lum = 1e-5 + LUM_W[0] * g[..., 0] + LUM_W[1] * g[..., 1] + LUM_W[2] * g[..., 2]
    out = g * (1.0 / lum)[..., None]
    return out, 2.0 * out.detach().numpy() * (1.0 + Sv)


def table(specs, x, pw):
    """Every filter's parameters from x [B, F, pw]: (table [B, F, pw] with zeros beyond n_f, S likewise)."""
    x = _t(x)
    rows, Ss = [], []
    for f, spec in enumerate(specs):
        out, S = regress(spec, x[:, f])
        rows.append(torch.nn.functional.pad(out, (0, pw - out.shape[-1])))
        Ss.append(np.pad(S, ((0, 0), (0, pw - S.shape[-1]))))
    return torch.stack(rows, dim=1), np.stack(Ss, axis=1)


def _pdf(logits, sc):
    sm = torch.softmax(logits, dim=1)
    p = (sm + 1e-37) * sc["one_minus_exploration"] + sc["exploration_over_f"]
    tot = torch.sum(p, dim=1, keepdim=True) + 1e-30
    return sm, tot, p / tot


def cdf_exclusive(pdf):
    """pdf_sample's exclusive CDF of a [B, F] pdf (numpy float64)."""
    q = pdf / (pdf.sum(axis=1, keepdims=True) + 1e-36)
    return np.cumsum(q, axis=1) - q


def select(pdf, u, forced_id, sample):
    """selected [B] int64: the forced id, or #{k : cdf_exclusive_k < u} - 1 (u == 0 gives -1), or the FIRST arg-max."""
    B = pdf.shape[0]
    if forced_id is not None and forced_id >= 0:
        return np.full(B, int(forced_id), dtype=np.int64)
    if sample:
        return (cdf_exclusive(pdf) < np.asarray(u, dtype=np.float64)[:, None]).sum(axis=1).astype(np.int64) - 1
    return np.argmax(pdf, axis=1).astype(np.int64)


def _tail_core(logits, states, sc, runtime, sel):
    """pdf, surrogate, penalty (torch, differentiable in logits), new_states and the penalty's parts with the selection given."""
    logits, states = _t(logits), _t(states)
    B, F = logits.shape
    sm, tot, pdf = _pdf(logits, sc)
    ent = torch.sum(-pdf * torch.log(pdf), dim=1)
    hot = torch.as_tensor((np.asarray(sel)[:, None] == np.arange(F)[None, :]).astype(np.float64))
    sur = torch.sum(hot * torch.log(pdf + 1e-10), dim=1)
    step, usage = states[:, 2], states[:, 3:]
    last = (torch.abs(step + 1.0 - sc["test_steps"]) < 1e-4).to(torch.float64)
    new_states = torch.cat([last[:, None], last[:, None], (step + 1.0)[:, None], torch.maximum(usage, hot)], dim=1)
    usage_pen = torch.sum(usage * hot, dim=1) * sc["filter_usage_penalty"]
    early = (1.0 - last) * last * sc["early_stop_penalty"]
    ent_pen = sc["entropy_coef"] * (-ent + sc["log_num_filters"])
    run_pen = torch.zeros(B, dtype=torch.float64)
    if runtime is not None:
        run_pen = sc["runtime_lambda"] * torch.sum(hot * _t(runtime)[None, :], dim=1)
    pen = ent_pen + usage_pen + early + run_pen
    return dict(sm=sm, tot=tot, pdf=pdf, surrogate=sur, penalty=pen, new_states=new_states, usage_pen=usage_pen, run_pen=run_pen)


def select_tail(logits, u, states, scalars, runtime, forced_id, sample):
    """The selector's tail of B images. logits [B, F], u [B], states [B, 3 + F]; `scalars` holds SCALAR_FIELDS (the values the
    argument struct carries) and "ops", the F op codes; runtime [F] or None; forced_id None / < 0 for none.
    Returns a dict: pdf, selected (int64), op_ids (int32), surrogate, new_states, penalty as numpy, and
      S_pdf       pdf max(1, |logit - max| / 16)
      S_surrogate |ref| + 1
      S_penalty   |coef| (sum p (|log p| + 1) + log F) + usage x penalty weight + |runtime term|."""
    sc = scalars
    lg = np.asarray(_t(logits).detach().numpy(), dtype=np.float64)
    with torch.no_grad():
        pdf = _pdf(_t(logits), sc)[2].numpy()
        sel = select(pdf, u, forced_id, sample)
        c = _tail_core(logits, states, sc, runtime, sel)
    F = lg.shape[1]
    ops = np.asarray(sc["ops"], dtype=np.int32)
    live = (sel >= 0) & (sel < F)
    sur, pen = c["surrogate"].numpy(), c["penalty"].numpy()
    S_pen = abs(sc["entropy_coef"]) * ((pdf * (np.abs(np.log(pdf)) + 1.0)).sum(axis=1) + abs(sc["log_num_filters"])) + \
        np.abs(c["usage_pen"].numpy()) + np.abs(c["run_pen"].numpy())
    return dict(pdf=pdf, S_pdf=pdf * np.maximum(1.0, np.abs(lg - lg.max(axis=1, keepdims=True)) / 16.0),
                selected=sel, op_ids=np.where(live, ops[np.clip(sel, 0, F - 1)], OP_ZERO).astype(np.int32),
                surrogate=sur, S_surrogate=np.abs(sur) + 1.0, new_states=c["new_states"].numpy(), penalty=pen, S_penalty=S_pen)


def packed(tab, S_tab, sel):
    """Row b = table[b, sel[b]] (zeros for an id outside 0..F-1), and its S."""
    B, F, pw = tab.shape
    live = ((sel >= 0) & (sel < F))[:, None]
    idx = np.clip(sel, 0, F - 1)
    return np.where(live, tab[np.arange(B), idx], 0.0), np.where(live, S_tab[np.arange(B), idx], 0.0)


def tail_backward(specs, x, logits, states, scalars, runtime, selected, d_packed=None, d_surrogate=None, d_penalty=None):
    """d_x [B, F, pw] and d_logits [B, F] by float64 autograd through `regress` and the tail with the selection held fixed, from
    d_packed [B, pw], d_surrogate [B], d_penalty [B] (None = absent). Returns (d_x, S_dx, d_logits, S_dlogits):

    S_dlogits is k_policy_tail_bwd's expression with every term replaced by its absolute value and every subtraction by an
    addition, |log p| + 2 for log p + 1 and 2 |dsur| / (p + 1e-10) for the surrogate term. S_dx per kind with dp the selected
    row's upstream gradient: TANH_RANGE |dp scale|; EXP_TANH_RANGE |dp scale| e^v (1 + S_v); SIGMOID |dp|; TANH 2 |dp|; WB the
    absolute-value form of regress_grad's expression times (1 + S_v)."""
    sc = scalars
    x64 = _t(x).clone().requires_grad_(True)
    lg64 = _t(logits).clone().requires_grad_(True)
    B, F, pw = x64.shape
    sel = np.asarray(selected, dtype=np.int64)
    live = (sel >= 0) & (sel < F)
    tab, _ = table(specs, x64, pw)
    c = _tail_core(lg64, states, sc, runtime, sel)
    loss = torch.zeros((), dtype=torch.float64)
    if d_packed is not None:
        idx = torch.as_tensor(np.clip(sel, 0, F - 1))
        rows = tab[torch.arange(B), idx] * torch.as_tensor(live.astype(np.float64))[:, None]
        loss = loss + torch.sum(rows * _t(d_packed))
    if d_surrogate is not None:
        loss = loss + torch.sum(c["surrogate"] * _t(d_surrogate))
    if d_penalty is not None:
        loss = loss + torch.sum(c["penalty"] * _t(d_penalty))
    if loss.requires_grad:
        gx, gl = torch.autograd.grad(loss, [x64, lg64], allow_unused=True)
    else:
        gx = gl = None
    d_x = np.zeros((B, F, pw)) if gx is None else gx.numpy()
    d_logits = np.zeros((B, F)) if gl is None else gl.numpy()

    # ---- S of d_logits
    sm, tot, pdf = (c[k].detach().numpy() for k in ("sm", "tot", "pdf"))
    dsur = np.zeros(B) if d_surrogate is None else np.abs(np.asarray(d_surrogate, dtype=np.float64))
    dpen = np.zeros(B) if d_penalty is None else np.abs(np.asarray(d_penalty, dtype=np.float64)) * abs(sc["entropy_coef"])
    hot = (sel[:, None] == np.arange(F)[None, :]).astype(np.float64)
    a_dpdf = dpen[:, None] * (np.abs(np.log(pdf)) + 2.0) + hot * 2.0 * dsur[:, None] / (pdf + 1e-10)
    a_dotp = (a_dpdf * pdf).sum(axis=1, keepdims=True)
    a_ds = (a_dpdf + a_dotp) / tot * abs(sc["one_minus_exploration"])
    S_dl = sm * (a_ds + (a_ds * sm).sum(axis=1, keepdims=True))

    # ---- S of d_x
    S_dx = np.zeros((B, F, pw))
    if d_packed is not None:
        dp_all = np.abs(np.asarray(d_packed, dtype=np.float64))
        xv = x64.detach().numpy()
        for b in range(B):
            if not live[b]:
                continue
            f = int(sel[b])
            n, kind, lo, scale, bias, Sv = spec_consts(specs[f])
            dp, r = dp_all[b, :n], xv[b, f, :n]
            if kind == KIND_SIGMOID:
                S = dp
            elif kind == KIND_TANH:
                S = 2.0 * dp
            elif kind == KIND_TANH_RANGE:
                S = dp * abs(scale)
            else:
                th = np.tanh(r * (np.array([0.0, 1.0, 1.0]) if kind == KIND_WB else 1.0) + bias)
                o = np.exp((th * 0.5 + 0.5) * scale + lo)
                if kind == KIND_EXP_TANH_RANGE:
                    S = dp * abs(scale) * o * (1.0 + Sv)
                else:
                    w = np.array(LUM_W)
                    lum = 1e-5 + (w * o).sum()
                    d_o = dp / lum + (dp * o).sum() / (lum * lum) * w
                    S = d_o * o * abs(scale) * 0.5 * (1.0 + th * th) * (1.0 + Sv)
                    S[0] = 0.0                                                   # the pinned R slot: exactly zero
            S_dx[b, f, :n] = S
    return d_x, S_dx, d_logits, S_dl


# ---- the training heads, one function per stage (csrc/isp_heads_train.hip) ----------------------------------------------------
def _np64(a):
    return np.asarray(a.detach().cpu().numpy() if isinstance(a, torch.Tensor) else a, dtype=np.float64)


def _slope(hidden):
    """LeakyReLU's slope per element, decided by the sign of the pre-activation given (the device's own `hidden`)."""
    return np.where(_np64(hidden) > 0, 1.0, 0.2)


def heads_fc1(feat_f, feat_s, w1, b1, ws1, bs1):
    """k_heads_fc1: hidden[b, g, j] = b1[g][j] + W1[g][j] . feat_g[b] (pre-activation; group F is the selector on feat_s).
    w1 / b1: lists of F arrays [hid, D] / [hid]. Returns (hidden, A) [B, F + 1, hid]; K = D."""
    feats = [_np64(feat_f)] * len(w1) + [_np64(feat_s)]
    ws, bs = [_np64(w) for w in w1] + [_np64(ws1)], [_np64(b) for b in b1] + [_np64(bs1)]
    pre = np.stack([f @ w.T + b for f, w, b in zip(feats, ws, bs)], axis=1)
    A = np.stack([np.abs(f) @ np.abs(w).T + np.abs(b) for f, w, b in zip(feats, ws, bs)], axis=1)
    return pre, A


def heads_out(hidden, wf, bf, ws2, bs2, pw):
    """k_heads_out: x[b, f, r] = bf[f][r] + Wf[f][r] . lrelu(hidden[b, f]) for r < n_f, 0 beyond; logits[b] from group F.
    Returns (x, A_x, logits, A_logits); K = hid."""
    h = _np64(hidden)
    act = h * _slope(h)
    B, F = h.shape[0], len(wf)
    x, Ax = np.zeros((B, F, pw)), np.zeros((B, F, pw))
    for f in range(F):
        w, b = _np64(wf[f]), _np64(bf[f])
        x[:, f, :w.shape[0]] = act[:, f] @ w.T + b
        Ax[:, f, :w.shape[0]] = np.abs(act[:, f]) @ np.abs(w).T + np.abs(b)
    w, b = _np64(ws2), _np64(bs2)
    return x, Ax, act[:, F] @ w.T + b, np.abs(act[:, F]) @ np.abs(w).T + np.abs(b)


def heads_dhid(hidden, dx, dlogits, wf, ws2):
    """k_heads_dhid, first part: dhid[b, g, h] = slope(hidden[b, g, h]) * sum_r W2[g][r][h] * up[b, g, r], up = dx[b, g, :n_g] or
    dlogits[b]. Returns (dhid, A) [B, F + 1, hid]; K = rows."""
    h, dx, dl = _np64(hidden), _np64(dx), _np64(dlogits)
    F = len(wf)
    out, A = np.zeros_like(h), np.zeros_like(h)
    for g in range(F + 1):
        w = _np64(wf[g] if g < F else ws2)
        up = dx[:, g, :w.shape[0]] if g < F else dl
        out[:, g], A[:, g] = up @ w, np.abs(up) @ np.abs(w)
    s = _slope(h)
    return out * s, A * s


def heads_dw2(hidden, dx, dlogits, n):
    """k_heads_dhid, second part: dW2[g][r][h] = sum_b up[b, g, r] * lrelu(hidden[b, g, h]), db2[g][r] = sum_b up[b, g, r].
    Returns lists over the F + 1 groups of (dW, A_dW, db, A_db); K = B."""
    h, dx, dl = _np64(hidden), _np64(dx), _np64(dlogits)
    act = h * _slope(h)
    F = len(n)
    res = []
    for g in range(F + 1):
        up = dx[:, g, :n[g]] if g < F else dl
        res.append((up.T @ act[:, g], np.abs(up).T @ np.abs(act[:, g]), up.sum(axis=0), np.abs(up).sum(axis=0)))
    return res


def heads_dw1(dhid, feat_f, feat_s):
    """k_heads_dw1: dW1[g][j][k] = sum_b dhid[b, g, j] * feat_g[b, k], db1[g][j] = sum_b dhid[b, g, j].
    Returns (dW1, A_dW1) [F + 1, hid, D] and (db1, A_db1) [F + 1, hid]; K = B."""
    d, ff, fs = _np64(dhid), _np64(feat_f), _np64(feat_s)
    G = d.shape[1]
    dW = np.stack([d[:, g].T @ (ff if g < G - 1 else fs) for g in range(G)])
    A = np.stack([np.abs(d[:, g]).T @ np.abs(ff if g < G - 1 else fs) for g in range(G)])
    return dW, A, d.sum(axis=0), np.abs(d).sum(axis=0)


def heads_dfeat(dhid, w1, ws1):
    """k_heads_dfeat_part + k_heads_dfeat_sum: dfeat_f[b] = sum_{g < F} dhid[b, g] @ W1[g] (K = hid + F: the longest chain),
    dfeat_s[b] = dhid[b, F] @ Ws1 (K = hid). Returns (dfeat_f, A_f, dfeat_s, A_s), each [B, D]."""
    d = _np64(dhid)
    F = len(w1)
    df = sum(d[:, g] @ _np64(w1[g]) for g in range(F))
    Af = sum(np.abs(d[:, g]) @ np.abs(_np64(w1[g])) for g in range(F))
    return df, Af, d[:, F] @ _np64(ws1), np.abs(d[:, F]) @ np.abs(_np64(ws1))
