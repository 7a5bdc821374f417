"""tests/_tailref.py is the float64 reference that tests/test_gpu_policy_tail.py and tests/test_gpu_heads_stages.py hold the
device to. Here, on the host:

  pin       it is the project's own ATen statement in double precision: Agent._heads_batched, the per-class regressors, and the
            selector lines of Agent.policy_heads with pdf_sample / one_hot — values and autograd gradients to 1e-12;
  headroom  a float32 numpy restatement of the kernels' operation order (csrc/isp_policy_math.h, k_policy_tail_bwd) uses at
            most a quarter of every bound on every case the device runs;
  mutants   each of thirteen deliberate errors in that restatement breaks a bound or a discrete output on a listed case;
  margins   no discrete output of a listed case hangs on fp32 rounding (tests/_tailcases.py: margins)."""
import math

import numpy as np
import pytest
import torch

import _tailcases as C
import _tailref as R

F32 = np.float32


# ---- pin -----------------------------------------------------------------------------------------------------------------------
def _agree(got, want, what):
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    assert got.shape == want.shape, what
    # 1e-12 relative; elements that cancel to almost nothing are held to 1e-12 of 1e-3 of the tensor's scale
    np.testing.assert_allclose(got, want, rtol=1e-12, atol=1e-15 * max(1.0, float(np.abs(want).max())), err_msg=what)


@pytest.fixture(scope="module")
def agent64():
    from _engine import cpu_agent
    from adaptiveisp_amd.config import cfg
    agent = cpu_agent(cfg).double()
    agent.runtime = agent.runtime.double()          # a plain attribute, not a buffer: .double() leaves it float32 (its values stay)
    return cfg, agent


def _pin_scalars(cfg, specs, coef):
    F = len(specs)
    return dict(one_minus_exploration=1 - cfg.exploration, exploration_over_f=cfg.exploration * 1.0 / F, entropy_coef=coef,
                log_num_filters=math.log(F), test_steps=cfg.test_steps, filter_usage_penalty=cfg.filter_usage_penalty,
                early_stop_penalty=cfg.early_stop_penalty, runtime_lambda=cfg.filter_runtime_penalty_lambda,
                ops=[int(s[0]) for s in specs])


def _pin_inputs(agent, B, seed):
    g = torch.Generator().manual_seed(seed)
    F, pw = len(agent.filters), agent._param_width
    x = torch.randn(B, F, pw, generator=g, dtype=torch.float64) * 2.0
    x[0, :, 0], x[B - 1, :, 0] = 30.0, -100.0
    for j, flt in enumerate(agent.filters):                                  # what _heads_pre gives: zeros in the padded slots
        x[:, j, flt.get_num_filter_parameters():] = 0.0
    logits = torch.randn(B, F, generator=g, dtype=torch.float64) * 3.0
    logits[1, 3] = logits[1].max() + 0.5
    logits[1, 7] = logits[1, 3]                                              # tied maxima: arg-max takes the first
    noise = torch.rand(B, 1, generator=g, dtype=torch.float64)
    noise[0, 0], noise[2, 0] = 0.0, 1.0                                      # id -1, and the last id
    states = torch.zeros(B, 3 + F, dtype=torch.float64)
    states[:, 2] = torch.tensor([4.0, 0.0, 4.00005, 3.9, 1.0, 4.0][:B], dtype=torch.float64)
    states[:, 3:] = (torch.rand(B, F, generator=g) < 0.5).double()
    x_down = torch.rand(B, 3, 64, 64, generator=g, dtype=torch.float64)
    return x.requires_grad_(True), logits.requires_grad_(True), noise, states, x_down


def test_regress_is_heads_batched_in_double(agent64):
    cfg, agent = agent64
    specs = [f.regressor_spec() for f in agent.filters]
    assert specs == C.production()
    x = _pin_inputs(agent, 6, 1)[0]
    w = torch.randn(x.shape, generator=torch.Generator().manual_seed(2), dtype=torch.float64)
    agent._heads_pre = lambda feats: x                                       # Agent._heads_batched on known pre-activations
    try:
        want = agent._heads_batched(torch.zeros(6, 1, dtype=torch.float64))
    finally:
        del agent._heads_pre
    got, S = R.table(specs, x, agent._param_width)
    _agree(got.detach(), want.detach(), "table")
    _agree(torch.autograd.grad((got * w).sum(), x)[0], torch.autograd.grad((want * w).sum(), x)[0], "d table / d x")
    assert S.shape == tuple(want.shape) and (S >= 0).all()
    for j, sp in enumerate(specs):
        assert (S[:, j, :sp[1]] > 0).all() and not S[:, j, sp[1]:].any()


@pytest.mark.parametrize("train,forced_id,runtime_on", [(True, None, False), (True, None, True), (True, 0, True), (True, 9, False),
                                                        (False, None, True), (False, None, False), (False, 4, False)])
def test_select_tail_and_backward_are_policy_heads_in_double(agent64, train, forced_id, runtime_on):
    cfg, agent = agent64
    specs = [f.regressor_spec() for f in agent.filters]
    F, pw, B, coef = len(specs), agent._param_width, 6, 0.7 * cfg.exploration_penalty
    x, logits, noise, states, x_down = _pin_inputs(agent, B, 3)
    hooks = [agent.fc2.register_forward_hook(lambda m, i, o: logits)]
    if train:
        agent._heads_pre = lambda feats: x
    else:                                                                    # eval: the per-class regressors on fc_filter's output
        for j, flt in enumerate(agent.filters):
            hooks.append(flt.fc_filter.register_forward_hook(
                lambda m, i, o, j=j, n=flt.get_num_filter_parameters(): x[:, j, :n]))
    saved = cfg.filter_runtime_penalty
    cfg.filter_runtime_penalty = runtime_on
    try:
        out = agent.policy_heads(x_down, noise, states, coef, train=train, forced_id=forced_id)
    finally:
        cfg.filter_runtime_penalty = saved
        for h in hooks:
            h.remove()
        if train:
            del agent._heads_pre
    pk, op_ids, selected, sur, pen, new_states, pdf, tab = out[:8]
    sc = _pin_scalars(cfg, specs, coef)
    runtime = agent.runtime.double().numpy() if runtime_on else None
    ref = R.select_tail(logits.detach(), noise[:, 0].numpy(), states, sc, runtime, forced_id, train)
    assert np.array_equal(ref["selected"], selected.numpy()) and np.array_equal(ref["op_ids"], op_ids.numpy())
    if forced_id is None:
        assert ref["selected"][1] == 3 or train                              # the first of the tied maxima
        assert not train or (ref["selected"][0] == -1 and ref["selected"][2] == F - 1)
    assert np.array_equal(ref["new_states"], new_states.numpy())
    _agree(ref["pdf"], pdf.detach(), "pdf")
    _agree(ref["surrogate"], sur.detach()[:, 0], "surrogate")
    _agree(ref["penalty"], pen.detach()[:, 0], "penalty")
    g = torch.Generator().manual_seed(4)
    dp, ds, dq = (torch.randn(s, generator=g, dtype=torch.float64) for s in ((B, pw), (B,), (B,)))
    # the packed row of id -1 is never read (op ZERO): the agent gathers row 0 there, the kernels write zeros
    live = torch.as_tensor((ref["selected"] >= 0).astype(np.float64))
    loss = (pk * dp * live[:, None]).sum() + (sur[:, 0] * ds).sum() + (pen[:, 0] * dq).sum()
    want_dx, want_dl = torch.autograd.grad(loss, [x, logits])
    if train:                                                                # eval regressors carry double constants, not the struct's
        got_tab, S_tab = R.table(specs, x.detach(), pw)
        _agree(got_tab, tab.detach(), "table")
        _agree(R.packed(got_tab.numpy(), S_tab, ref["selected"])[0], (pk.detach() * live[:, None]), "packed")
    d_x, S_dx, d_l, S_dl = R.tail_backward(specs, x.detach(), logits.detach(), states, sc, runtime, ref["selected"],
                                            dp.numpy(), ds.numpy(), dq.numpy())
    _agree(d_l, want_dl, "d_logits")
    if train:
        _agree(d_x, want_dx, "d_x")
    else:
        np.testing.assert_allclose(d_x, want_dx.numpy(), rtol=1e-6, atol=1e-9)
    assert (S_dx >= 0).all() and (S_dl >= 0).all()
    # absent upstream gradients are zeros
    z = R.tail_backward(specs, x.detach(), logits.detach(), states, sc, runtime, ref["selected"])
    assert not z[0].any() and not z[2].any() and not z[1].any() and not z[3].any()


# ---- the float32 restatement ---------------------------------------------------------------------------------------------------
def _seq_sum(cols):
    s = np.zeros(cols.shape[0], dtype=F32)
    for k in range(cols.shape[1]):
        s = s + cols[:, k]
    return s


def _tanh01(v):
    return np.tanh(v) * F32(0.5) + F32(0.5)


def _consts(spec, mutant):
    _, n, kind, lo, scale, bias = spec
    return n, kind, F32(lo), F32(scale), F32(0.0 if mutant == "bias dropped" else bias)


def _lum(o, mutant):
    w = (0.67, 0.06, 0.27) if mutant == "luminance weights permuted" else R.LUM_W
    return ((F32(1e-5) + F32(w[0]) * o[..., 0]) + F32(w[1]) * o[..., 1]) + F32(w[2]) * o[..., 2]


def regress32(spec, row, mutant=None):
    """regress of isp_policy_math.h on rows [B, >= n] float32 -> [B, n]."""
    n, kind, lo, scale, bias = _consts(spec, mutant)
    x = row[:, :n]
    if kind == R.KIND_SIGMOID:
        return F32(1.0) / (F32(1.0) + np.exp(-x))
    if kind == R.KIND_TANH:
        return np.tanh(x)
    if kind == R.KIND_WB:
        keep = np.array([1.0 if mutant == "white balance keeps R" else 0.0, 1.0, 1.0], dtype=F32)
        g = np.exp(_tanh01(x * keep + bias) * scale + lo)
        return g * (F32(1.0) / _lum(g, mutant))[:, None]
    v = _tanh01(x + bias) * scale + lo
    return v if kind == R.KIND_TANH_RANGE else np.exp(v)


def regress_grad32(spec, row, dp, mutant=None):
    """regress_grad on one row [>= n] with the parameter row's gradient dp [>= n] -> [n]."""
    n, kind, lo, scale, bias = _consts(spec, mutant)
    x, dp = row[:n], dp[:n]
    one = F32(1.0)
    dth = (lambda th: one - th) if mutant == "1 - th in regress_grad" else (lambda th: one - th * th)
    if kind == R.KIND_TANH_RANGE:
        return dp * scale * F32(0.5) * dth(np.tanh(x + bias))
    if kind == R.KIND_EXP_TANH_RANGE:
        th = np.tanh(x + bias)
        return dp * np.exp((th * F32(0.5) + F32(0.5)) * scale + lo) * scale * F32(0.5) * dth(th)
    if kind == R.KIND_SIGMOID:
        sg = one / (one + np.exp(-x))
        return dp * sg * (one - sg)
    if kind == R.KIND_TANH:
        return dp * dth(np.tanh(x))
    th = np.tanh(x * np.array([0.0, 1.0, 1.0], dtype=F32) + bias)
    o = np.exp((th * F32(0.5) + F32(0.5)) * scale + lo)
    lum = _lum(o, None)
    w = np.array(R.LUM_W, dtype=F32)
    dot = F32(0.0)
    for c in range(3):
        dot = dot + dp[c] * o[c]
    d_o = dp / lum - (F32(0.0) if mutant == "white balance coupling dropped" else dot / (lum * lum) * w)
    out = d_o * o * scale * F32(0.5) * dth(th)
    out[0] = F32(0.0)
    return out


def forward32(case, mutant=None):
    """k_policy_tail_fwd (and k_finish after its dot products) in float32 numpy, in the kernels' operation order."""
    specs, sc, F, pw, B = case["specs"], case["scalars"], case["F"], case["pw"], case["B"]
    x, lg, u, st = case["x"], case["logits"], case["u"], case["states"]
    with np.errstate(over="ignore", under="ignore", divide="ignore", invalid="ignore"):
        tab = np.zeros((B, F, pw), dtype=F32)
        for f, spec in enumerate(specs):
            tab[:, f, :spec[1]] = regress32(spec, x[:, f], mutant)
        ome, eof = F32(sc["one_minus_exploration"]), F32(sc["exploration_over_f"])
        e = np.exp(lg - lg.max(axis=1, keepdims=True))
        pdf = e / _seq_sum(e)[:, None] + F32(1e-37)
        if mutant != "exploration mix omitted":
            pdf = pdf * ome + eof
        p = pdf / (_seq_sum(pdf) + F32(1e-30))[:, None]
        entl = -p * np.log(p)
        if mutant == "entropy sign flipped":
            entl = -entl
        ent = _seq_sum(entl)
        s2 = _seq_sum(p) + F32(1e-36)
        cnt, amax, run = np.zeros(B, dtype=np.int64), np.zeros(B, dtype=np.int64), np.zeros(B, dtype=F32)
        rows = np.arange(B)
        for k in range(F):
            pk = p[:, k] / s2
            run = run + pk
            cnt += (run if mutant == "inclusive CDF" else run - pk) < u
            better = p[:, k] >= p[rows, amax] if mutant == "arg-max takes the last" else p[:, k] > p[rows, amax]
            amax = np.where(better, k, amax)
        sel = np.full(B, case["forced_id"]) if case["forced_id"] >= 0 else (cnt - 1 if case["sample"] else amax)
        live = (sel >= 0) & (sel < F)
        idx = np.clip(sel, 0, F - 1)
        ops = np.where(live, np.asarray(sc["ops"], dtype=np.int32)[idx], R.OP_ZERO).astype(np.int32)
        psel = p[rows, idx]
        sur = np.where(live, np.log(psel if mutant == "+1e-10 dropped" else psel + F32(1e-10)), F32(0.0)).astype(F32)
        T = F32(sc["test_steps"])
        if mutant == "last-step window is equality":
            last = ((st[:, 2] + F32(1.0)) == T).astype(F32)
        else:
            last = (np.abs(st[:, 2] + F32(1.0) - T) < F32(1e-4)).astype(F32)
        ns = np.zeros((B, 3 + F), dtype=F32)
        ns[:, 0], ns[:, 1], ns[:, 2] = last, last, st[:, 2] + F32(1.0)
        hot = (sel[:, None] == np.arange(F)[None, :]).astype(F32)
        usage_pen = _seq_sum(st[:, 3:] * hot)
        if mutant == "usage penalty omitted":
            usage_pen = usage_pen * F32(0.0)
        ns[:, 3:] = hot if mutant == "usage flags overwritten" else np.maximum(st[:, 3:], hot)
        ent_pen = F32(sc["entropy_coef"]) * (-ent + F32(sc["log_num_filters"]))
        early = (F32(1.0) - last) * last * F32(sc["early_stop_penalty"])
        run_pen = np.zeros(B, dtype=F32)
        if case["runtime"] is not None:
            run_pen = np.where(live, F32(sc["runtime_lambda"]) * case["runtime"][idx], F32(0.0)).astype(F32)
        pen = F32(0.0) + ent_pen + usage_pen * F32(sc["filter_usage_penalty"]) + early + run_pen
        packed = np.where(live[:, None], tab[rows, idx], F32(0.0)).astype(F32)
    return dict(table=tab, packed=packed, pdf=p, selected=sel, op_ids=ops, surrogate=sur, new_states=ns, penalty=pen)


def backward32(case, pdf, sel, d_packed, d_surrogate, d_penalty, mutant=None):
    """k_policy_tail_bwd in float32 numpy on the forward's pdf and selection."""
    specs, sc, F, pw, B = case["specs"], case["scalars"], case["F"], case["pw"], case["B"]
    x, lg = case["x"], case["logits"]
    live = (sel >= 0) & (sel < F)
    dx = np.zeros((B, F, pw), dtype=F32)
    with np.errstate(over="ignore", under="ignore", divide="ignore", invalid="ignore"):
        if d_packed is not None:
            for b in np.nonzero(live)[0]:
                f = int(sel[b])
                dx[b, f, :specs[f][1]] = regress_grad32(specs[f], x[b, f], d_packed[b], mutant)
        ome, eof = F32(sc["one_minus_exploration"]), F32(sc["exploration_over_f"])
        sm = np.exp(lg - lg.max(axis=1, keepdims=True))
        sm = sm / _seq_sum(sm)[:, None]
        tot = _seq_sum((sm + F32(1e-37)) * ome + eof) + F32(1e-30)
        dsur = np.zeros(B, dtype=F32) if d_surrogate is None else d_surrogate
        dpen = (np.zeros(B, dtype=F32) if d_penalty is None else d_penalty) * F32(sc["entropy_coef"])
        hot = live[:, None] & (sel[:, None] == np.arange(F)[None, :])
        dpdf = dpen[:, None] * (np.log(pdf) + F32(1.0))
        dpdf = np.where(hot, dpdf + dsur[:, None] / (pdf + F32(1e-10)), dpdf).astype(F32)
        dotp = _seq_sum(dpdf * pdf)
        ds = (dpdf - dotp[:, None]) / tot[:, None] * ome
        dots = _seq_sum(ds * sm)
        dl = sm * (ds - dots[:, None])
    return dx, dl.astype(F32)


MUTANTS = ["bias dropped", "white balance keeps R", "luminance weights permuted", "exploration mix omitted", "+1e-10 dropped",
           "entropy sign flipped", "arg-max takes the last", "inclusive CDF", "last-step window is equality",
           "usage penalty omitted", "usage flags overwritten", "1 - th in regress_grad", "white balance coupling dropped"]


def _share(got, ref, S):
    a, b = R.normalised(got, ref, S)
    return float(np.abs(a - b).max() / R.CAP) if a.size else 0.0


_REF = {}


def _reference(case):
    """The float64 side of a case, computed once."""
    if case["name"] not in _REF:
        fwd = R.select_tail(case["logits"], case["u"], case["states"], case["scalars"], case["runtime"], case["forced_id"],
                            case["sample"])
        tab, S_tab = R.table(case["specs"], case["x"], case["pw"])
        fwd["table"], fwd["S_table"] = tab.numpy(), S_tab
        fwd["packed"], fwd["S_packed"] = R.packed(fwd["table"], S_tab, fwd["selected"])
        bwd = R.tail_backward(case["specs"], case["x"], case["logits"], case["states"], case["scalars"], case["runtime"],
                              fwd["selected"], *C.upstream(case))
        _REF[case["name"]] = (fwd, bwd)
    return _REF[case["name"]]


def _shares(case, mutant=None):
    """{output: share of its bound the float32 restatement uses}, math.inf where a discrete output differs."""
    fwd, bwd = _reference(case)
    got = forward32(case, mutant)
    out = {k: 0.0 if np.array_equal(got[k], fwd[k].astype(got[k].dtype)) else math.inf
           for k in ("selected", "op_ids", "new_states")}
    for k in ("table", "packed", "pdf", "surrogate", "penalty"):
        out[k] = _share(got[k], fwd[k], fwd["S_" + k])
    if out["selected"] == 0.0:                                               # the backward runs on the forward's own selection
        dx, dl = backward32(case, got["pdf"], got["selected"], *C.upstream(case), mutant=mutant)
        out["d_x"], out["d_logits"] = _share(dx, bwd[0], bwd[1]), _share(dl, bwd[2], bwd[3])
        assert mutant or not dx[bwd[1] == 0].any()
    return out


def _all_cases():
    return C.tail_cases() + C.finish_cases()


def test_case_list_covers_what_the_device_tests_claim():
    tail, fin = C.tail_cases(), C.finish_cases()
    names = [c["name"] for c in tail + fin]
    assert len(set(names)) == len(names)
    for tag, F in (("prod10", 10), ("f1", 1), ("f2", 2), ("f16", 16)):
        mine = [c for c in tail if c["name"][3:].startswith(tag + "-")]
        assert {c["B"] for c in mine} >= {1, 3, 9, 70} and all(c["F"] == F for c in mine)
    assert {c["exploration"] for c in tail} == {0.0, 0.05, 1.0} and {c["noise_stride"] for c in tail} == {1, 2}
    assert {(c["forced_id"] < 0, c["forced_id"] == 0, c["sample"]) for c in tail if c["F"] > 1} >= \
        {(True, False, 1), (True, False, 0), (False, True, 1), (False, True, 0), (False, False, 1), (False, False, 0)}
    assert {c["runtime"] is None for c in tail} == {True, False}
    u = np.concatenate([c["u"] for c in tail if c["sample"] and c["forced_id"] < 0])
    assert {0.0, float(F32(1e-7)), float(F32(0.999999)), 1.0} <= set(u.tolist())
    steps = np.concatenate([c["states"][:, 2] for c in tail])
    assert {float(F32(s)) for s in C.STEPS} <= set(steps.tolist())
    for c in tail:
        d = np.abs(c["logits"] - c["logits"].max(axis=1, keepdims=True))
        assert ((d <= 40.0) | (c["logits"] == -120.0)).all()
    assert any((c["logits"] == -120.0).any() for c in tail) and any(np.abs(c["x"]).max() == 100.0 for c in tail)
    ties = [c for c in tail if not c["sample"] and c["forced_id"] < 0 and
            ((c["logits"] == c["logits"].max(axis=1, keepdims=True)).sum(axis=1) == 2).any()]
    assert ties, "no unforced arg-max over two bit-equal maxima"
    for kind in range(5):                                                    # +-30 and +-100 in every kind
        seen = set()
        for c in tail:
            for f, sp in enumerate(c["specs"]):
                if sp[2] == kind:
                    seen |= set(np.abs(c["x"][:, f, :sp[1]]).ravel().tolist()) & {30.0, 100.0}
        assert seen == {30.0, 100.0}, kind
    assert {(c["hid"], c["row_filter"].size + c["F"]) for c in fin} >= {(8, 37), (72, 2), (128, 96), (128, 97), (72, 400), (256, 29),
                                                                      (264, 37), (320, 29)}


def test_every_case_keeps_its_decision_margins():
    for c in _all_cases():
        ok = C.margins(c["logits"], c["u"], c["states"][:, 2], c["scalars"], c["sample"])
        assert ok.all(), f"{c['name']}: images {np.nonzero(~ok)[0].tolist()}"


def test_float32_restatement_uses_a_quarter_of_each_bound():
    worst = {}
    for c in _all_cases():
        for k, v in _shares(c).items():
            if v > worst.get(k, (-1.0, ""))[0]:
                worst[k] = (v, c["name"])
    print({k: (round(v, 4), n) for k, (v, n) in worst.items()})
    bad = {k: v for k, v in worst.items() if not v[0] <= 0.25}
    assert not bad, f"float32 arithmetic in the kernels' order uses more than 0.25 of the bound: {bad}"


@pytest.mark.parametrize("mutant", MUTANTS)
def test_mutant_breaks_a_bound_or_a_discrete_output(mutant):
    for c in _all_cases():
        hit = {k: v for k, v in _shares(c, mutant).items() if v > 1.0}
        if hit:
            print(f"{mutant}: {c['name']} {hit}")
            return
    raise AssertionError(f"'{mutant}' passes every bound on every listed case")


# ---- the heads stages' references -------------------------------------------------------------------------------------------------
def test_heads_stage_references_chain_to_float64_autograd():
    """The seven stage functions, each fed the previous one's output, give the gradients autograd gives for the same network."""
    rng = np.random.default_rng(5)
    B, F, D, hid, pw, n = 3, 3, 16, 8, 4, [4, 1, 2]
    t = lambda *s: torch.from_numpy(rng.normal(size=s)).requires_grad_(True)  # noqa: E731
    ff, fs = t(B, D), t(B, D)
    w1, b1, wf, bf = [t(hid, D) for _ in n], [t(hid) for _ in n], [t(k, hid) for k in n], [t(k) for k in n]
    ws1, bs1, ws2, bs2 = t(hid, D), t(hid), t(F, hid), t(F)
    lin, act = torch.nn.functional.linear, lambda v: torch.nn.functional.leaky_relu(v, 0.2)  # noqa: E731
    hidden = torch.stack([lin(ff, w1[g], b1[g]) for g in range(F)] + [lin(fs, ws1, bs1)], dim=1)
    x = torch.stack([torch.nn.functional.pad(lin(act(hidden[:, g]), wf[g], bf[g]), (0, pw - n[g])) for g in range(F)], dim=1)
    logits = lin(act(hidden[:, F]), ws2, bs2)
    dx, dl = rng.normal(size=(B, F, pw)), rng.normal(size=(B, F))
    leaves = [ff, fs] + w1 + b1 + wf + bf + [ws1, bs1, ws2, bs2]
    grads = torch.autograd.grad((x * torch.from_numpy(dx)).sum() + (logits * torch.from_numpy(dl)).sum(), leaves)
    gd = dict(zip(range(len(leaves)), (g.numpy() for g in grads)))
    h, A = R.heads_fc1(ff, fs, w1, b1, ws1, bs1)
    np.testing.assert_allclose(h, hidden.detach().numpy(), rtol=1e-12, atol=1e-13)
    assert (A >= np.abs(h)).all()
    gx, Ax, gl, Al = R.heads_out(h, wf, bf, ws2, bs2, pw)
    np.testing.assert_allclose(gx, x.detach().numpy(), rtol=1e-12, atol=1e-13)
    np.testing.assert_allclose(gl, logits.detach().numpy(), rtol=1e-12, atol=1e-13)
    assert (Ax >= np.abs(gx)).all() and (Al >= np.abs(gl)).all() and not Ax[:, 1, 1:].any()
    dhid, Ad = R.heads_dhid(h, dx, dl, wf, ws2)
    assert (Ad >= np.abs(dhid) - 1e-12).all()
    dW1, AW, db1, Ab = R.heads_dw1(dhid, ff, fs)
    dff, Af, dfs, As = R.heads_dfeat(dhid, w1, ws1)
    w2 = R.heads_dw2(h, dx, dl, n)
    o = 2
    want = dict(ff=gd[0], fs=gd[1], w1=[gd[o + g] for g in range(F)], b1=[gd[o + F + g] for g in range(F)],
                wf=[gd[o + 2 * F + g] for g in range(F)], bf=[gd[o + 3 * F + g] for g in range(F)],
                ws1=gd[o + 4 * F], bs1=gd[o + 4 * F + 1], ws2=gd[o + 4 * F + 2], bs2=gd[o + 4 * F + 3])
    tol = dict(rtol=1e-11, atol=1e-12)
    np.testing.assert_allclose(dff, want["ff"], **tol)
    np.testing.assert_allclose(dfs, want["fs"], **tol)
    for g in range(F):
        np.testing.assert_allclose(dW1[g], want["w1"][g], **tol)
        np.testing.assert_allclose(db1[g], want["b1"][g], **tol)
        np.testing.assert_allclose(w2[g][0], want["wf"][g], **tol)
        np.testing.assert_allclose(w2[g][2], want["bf"][g], **tol)
    np.testing.assert_allclose(dW1[F], want["ws1"], **tol)
    np.testing.assert_allclose(db1[F], want["bs1"], **tol)
    np.testing.assert_allclose(w2[F][0], want["ws2"], **tol)
    np.testing.assert_allclose(w2[F][2], want["bs2"], **tol)
    assert (AW >= np.abs(dW1) - 1e-12).all() and (Af >= np.abs(dff) - 1e-12).all() and (As >= np.abs(dfs) - 1e-12).all()
    assert (Ab >= np.abs(db1) - 1e-12).all() and all((r[1] >= np.abs(r[0]) - 1e-12).all() for r in w2)
