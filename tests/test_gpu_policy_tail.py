"""adaisp_policy_finish (csrc/isp_policy.hip: k_finish) and adaisp_policy_tail_fwd / _bwd (csrc/isp_rl_train.hip) through the C ABI
against the float64 restatement of tests/_tailref.py (pinned to the ATen statements by tests/test_tailref_host.py), on the cases
of tests/_tailcases.py: four regressor tables (F = 1, 2, 10, 16; widths 1 to 24; non-zero regressor biases), B = 1 to 70,
saturated pre-activations, tied maxima, a -120 logit, exploration 0 / 0.05 / 1, u = 0 / 1e-7 / 0.999999 / 1, forced ids, the
last-step window's edges, the runtime table given and absent, both noise strides.

Discrete outputs (selected, op_ids, new_states) equal the reference exactly: the host test asserts for every case that none of
them hangs on fp32 rounding. Float outputs satisfy |got - ref| <= CAP * S + 1e-30 with the magnitudes S of _tailref; CAP = 1e-5
is the project's cap for fp32 arithmetic through device transcendentals, not a measurement of the device. k_finish gets its
pre-activations from lattice inputs, so its dot products are exact in any order and the same reference applies to it; its row
loop (more than 96 rows) and its hidden loop (hid > 256) are run here. Every launch runs twice and must repeat its bits; every
output sits between NaN guards."""
import ctypes
import itertools

import numpy as np
import pytest
import torch

import _tailcases as C
import _tailref as R
from _margins import close

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
GUARD = 256                     # 32-bit words before and after every output
ESHAPE = -4                     # ADAISP_ESHAPE (include/adaisp.h)
FILL = np.array([np.nan], dtype=np.float32).view(np.uint32)[0]


@pytest.fixture(scope="module")
def L():
    from adaptiveisp_amd import _lib
    from adaptiveisp_amd.policy_fast import _FinishArgs
    from adaptiveisp_amd.policy_train import _TailArgs
    lib = _lib.load()
    lib.adaisp_policy_finish.argtypes = [ctypes.POINTER(_FinishArgs), ctypes.c_int, ctypes.c_void_p]
    lib.adaisp_policy_tail_fwd.argtypes = lib.adaisp_policy_tail_bwd.argtypes = [ctypes.POINTER(_TailArgs), ctypes.c_void_p]
    lib.adaisp_policy_finish.restype = lib.adaisp_policy_tail_fwd.restype = lib.adaisp_policy_tail_bwd.restype = ctypes.c_int
    return lib


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


class _Guarded:
    """An output of `shape` and dtype between two NaN-filled guards; the output itself starts as the same fill."""

    def __init__(self, shape, dtype=np.float32):
        self.shape, self.dtype = tuple(shape), np.dtype(dtype)
        self.words = int(np.prod(self.shape)) * self.dtype.itemsize // 4
        self.buf = torch.full((GUARD + self.words + GUARD,), float("nan"), dtype=torch.float32, device=DEV)
        self.ptr = self.buf.data_ptr() + 4 * GUARD

    def read(self, what, partial=False):
        h = self.buf.cpu().numpy().view(np.uint32)
        assert (h[:GUARD] == FILL).all() and (h[GUARD + self.words:] == FILL).all(), f"{what}: wrote outside its output"
        body = h[GUARD:GUARD + self.words].copy()
        if not partial:
            assert not (body == FILL).any(), f"{what}: {int((body == FILL).sum())} of {self.words} words not written"
        out = body.view(self.dtype).reshape(self.shape)
        assert partial or self.dtype != np.float32 or not np.isnan(out).any(), f"{what}: NaN"
        return out

    def untouched(self):
        return bool((self.buf.cpu().numpy().view(np.uint32) == FILL).all())


def _shared(a, case, sample_field, ins):
    from adaptiveisp_amd.policy_fast import _Regressor
    sc = case["scalars"]
    a.num_filters, a.param_width, a.noise_stride, a.forced_id = case["F"], case["pw"], case["noise_stride"], case["forced_id"]
    setattr(a, sample_field, case["sample"])
    for k in R.SCALAR_FIELDS:
        setattr(a, k, sc[k])
        assert getattr(a, k) == sc[k], k                                     # the struct carries the value the reference uses
    for j, spec in enumerate(case["specs"]):
        a.reg[j] = _Regressor(*spec)
    ins["noise"], ins["states"] = _dev(case["noise"]), _dev(case["states"])
    a.noise, a.states = ins["noise"].data_ptr(), ins["states"].data_ptr()
    if case["runtime"] is not None:
        ins["runtime"] = _dev(case["runtime"])
    a.runtime = ins["runtime"].data_ptr() if case["runtime"] is not None else None


def _outputs(case, table_name):
    B, F, pw = case["B"], case["F"], case["pw"]
    return {table_name: _Guarded((B, F, pw)), "packed": _Guarded((B, pw)), "op_ids": _Guarded((B,), np.int32),
            "selected": _Guarded((B,), np.int64), "pdf": _Guarded((B, F)), "surrogate": _Guarded((B,)),
            "new_states": _Guarded((B, 3 + F)), "penalty": _Guarded((B,))}


def _read(outs, what, partial=()):
    return {k: o.read(f"{what} {k}", partial=k in partial) for k, o in outs.items()}


def _same_bits(a, b, what):
    for k in a:
        assert np.array_equal(a[k].view(np.uint8), b[k].view(np.uint8)), f"{what}: {k} differs between two launches"


def _tail_fwd(L, case):
    """Two launches on the same inputs; returns (host outputs, the first launch's device outputs, args, inputs)."""
    from adaptiveisp_amd import _lib
    from adaptiveisp_amd.policy_train import _TailArgs
    runs = []
    with torch.cuda.device(DEV):
        for _ in range(2):
            a, ins = _TailArgs(), {}
            _shared(a, case, "sample", ins)
            ins["x"], ins["logits"] = _dev(case["x"]), _dev(case["logits"])
            a.B, a.x, a.logits = case["B"], ins["x"].data_ptr(), ins["logits"].data_ptr()
            outs = _outputs(case, "table")
            for k, o in outs.items():
                setattr(a, k, o.ptr)
            _lib._check(L.adaisp_policy_tail_fwd(ctypes.byref(a), _lib._stream()), "adaisp_policy_tail_fwd")
            torch.cuda.synchronize()
            runs.append((_read(outs, f"adaisp_policy_tail_fwd {case['name']}"), outs, a, ins))
    _same_bits(runs[0][0], runs[1][0], case["name"])
    return runs[0]


def _tail_bwd(L, case, fwd, grads):
    from adaptiveisp_amd import _lib
    _, outs, a, ins = fwd
    runs = []
    with torch.cuda.device(DEV):
        for _ in range(2):
            keep = [None if g is None else _dev(g) for g in grads]
            a.d_packed, a.d_surrogate, a.d_penalty = (None if g is None else g.data_ptr() for g in keep)
            o = {"d_x": _Guarded((case["B"], case["F"], case["pw"])), "d_logits": _Guarded((case["B"], case["F"]))}
            a.d_x, a.d_logits = o["d_x"].ptr, o["d_logits"].ptr
            _lib._check(L.adaisp_policy_tail_bwd(ctypes.byref(a), _lib._stream()), "adaisp_policy_tail_bwd")
            torch.cuda.synchronize()
            runs.append(_read(o, f"adaisp_policy_tail_bwd {case['name']}"))
    _same_bits(runs[0], runs[1], case["name"] + " backward")
    for k, o in outs.items():                                                # the backward writes none of the forward's outputs
        o.read(f"{case['name']} {k} after the backward")
    return runs[0]


def _finish(L, case):
    from adaptiveisp_amd import _lib
    from adaptiveisp_amd.policy_fast import _FinishArgs
    runs = []
    with torch.cuda.device(DEV):
        for _ in range(2):
            a, ins = _FinishArgs(), {}
            _shared(a, case, "train_mode", ins)
            for k in ("hidden", "w_filter", "b_filter", "row_filter", "row_slot", "w_sel", "b_sel"):
                ins[k] = _dev(case[k])
                setattr(a, k, ins[k].data_ptr())
            a.num_rows, a.hid = case["row_filter"].size, case["hid"]
            outs = _outputs(case, "params_all")
            for k, o in outs.items():
                setattr(a, "pdf_out" if k == "pdf" else k, o.ptr)
            _lib._check(L.adaisp_policy_finish(ctypes.byref(a), case["B"], _lib._stream()), "adaisp_policy_finish")
            torch.cuda.synchronize()
            got = _read(outs, f"adaisp_policy_finish {case['name']}", partial=("params_all",))
            got["table"] = got.pop("params_all")
            runs.append(got)
    _same_bits(runs[0], runs[1], case["name"])
    return runs[0]


def _reference(case):
    ref = R.select_tail(case["logits"], case["u"], case["states"], case["scalars"], case["runtime"], case["forced_id"],
                        case["sample"])
    tab, S_tab = R.table(case["specs"], case["x"], case["pw"])
    ref["table"], ref["S_table"] = tab.numpy(), S_tab
    ref["packed"], ref["S_packed"] = R.packed(ref["table"], S_tab, ref["selected"])
    return ref


def _bounded(label, got, ref, S, what):
    g, r = R.normalised(got, ref, S)
    share = float(np.abs(g - r).max() / R.CAP) if g.size else 0.0
    print(f"{what} {label}: {share:.4f} of its bound")
    close(label, g, r, rtol=0, atol=R.CAP, err_msg=what)


def _check_forward(prefix, case, got, ref, table_beyond_n):
    what, F = case["name"], case["F"]
    sel = ref["selected"]
    assert np.array_equal(got["selected"], sel), f"{what}: selected {got['selected'].tolist()} vs {sel.tolist()}"
    assert np.array_equal(got["op_ids"], ref["op_ids"]), f"{what}: op_ids"
    assert np.array_equal(got["new_states"], ref["new_states"].astype(np.float32)), f"{what}: new_states"
    valid = np.zeros((F, case["pw"]), dtype=bool)
    for f, sp in enumerate(case["specs"]):
        valid[f, :sp[1]] = True
    if table_beyond_n:
        assert not got["table"][:, ~valid].view(np.uint32).any(), f"{what}: table beyond n_f is not +0"
    _bounded(prefix + ".table", got["table"][:, valid], ref["table"][:, valid], ref["S_table"][:, valid], what)
    live = (sel >= 0) & (sel < F)
    dead = ~valid[np.clip(sel, 0, F - 1)] | ~live[:, None]                   # [B, pw]: beyond the selected n, or id -1
    assert not got["packed"][dead].view(np.uint32).any(), f"{what}: packed outside the selected parameters is not +0"
    _bounded(prefix + ".packed", got["packed"], ref["packed"], ref["S_packed"], what)
    for k in ("pdf", "surrogate", "penalty"):
        _bounded(f"{prefix}.{k}", got[k], ref[k], ref["S_" + k], what)
    if case["sample"] and case["forced_id"] < 0:                            # the designed u = 0: an all-zero one-hot
        z = case["u"] == 0.0
        assert (sel[z] == -1).all() and (got["op_ids"][z] == R.OP_ZERO).all() and not got["surrogate"][z].view(np.uint32).any()
        assert np.array_equal(got["new_states"][z, 3:], case["states"][z, 3:])
        assert (sel[case["u"] == 1.0] == F - 1).all()


@pytest.mark.parametrize("tag", ["prod10", "f1", "f2", "f16"])
def test_tail_forward_against_float64(L, tag):
    cases = [c for c in C.tail_cases() if c["name"][3:].startswith(tag + "-")]
    assert len(cases) >= 8
    for case in cases:
        got, *_ = _tail_fwd(L, case)
        _check_forward("policy_tail", case, got, _reference(case), table_beyond_n=True)


@pytest.mark.parametrize("tag", ["prod10", "f1", "f2", "f16"])
def test_tail_backward_against_float64_autograd(L, tag):
    cases = [c for c in C.tail_cases() if c["name"][3:].startswith(tag + "-")]
    for case in cases:
        fwd = _tail_fwd(L, case)
        got_f, F, what = fwd[0], case["F"], case["name"]
        sel = got_f["selected"]
        assert np.array_equal(sel, _reference(case)["selected"])
        live = (sel >= 0) & (sel < F)
        up = C.upstream(case)
        for mask in itertools.product((False, True), repeat=3):              # every combination of NULL and given
            grads = [g if m else None for g, m in zip(up, mask)]
            got = _tail_bwd(L, case, fwd, grads)
            d_x, S_dx, d_l, S_dl = R.tail_backward(case["specs"], case["x"], case["logits"], case["states"], case["scalars"],
                                                   case["runtime"], sel, *grads)
            # +0 outside the selected row, beyond n_f, everywhere for id -1 and in the white balance's slot 0: where S is 0
            structural = np.ones(d_x.shape, dtype=bool)
            for b in np.nonzero(live)[0]:
                sp = case["specs"][sel[b]]
                structural[b, sel[b], (1 if sp[2] == R.KIND_WB else 0):sp[1]] = False
            assert not S_dx[structural].any()
            assert not got["d_x"][structural].view(np.uint32).any(), f"{what} {mask}: d_x is not +0 where nothing flows"
            if not mask[0]:
                assert not got["d_x"].view(np.uint32).any(), f"{what}: d_x without d_packed"
            _bounded("policy_tail.d_x", got["d_x"], d_x, S_dx, f"{what} {mask}")
            _bounded("policy_tail.d_logits", got["d_logits"], d_l, S_dl, f"{what} {mask}")
            if case["exploration"] == 1.0:
                assert not S_dl.any() and (got["d_logits"] == 0.0).all(), f"{what}: d_logits with exploration 1"


@pytest.mark.parametrize("i", range(len(C.FINISH_SHAPES)), ids=["-".join(str(v) for v in s) for s in C.FINISH_SHAPES])
def test_finish_against_float64(L, i):
    case = C.finish_cases()[i]
    assert (case["row_filter"].size + case["F"] <= 96 and case["hid"] <= 256) == (i not in (5, 6, 7, 8)), "register / loop path"
    got = _finish(L, case)
    _check_forward("policy_finish", case, got, _reference(case), table_beyond_n=False)       # params_all: s < n_f only


# ---- error paths -----------------------------------------------------------------------------------------------------------------
def _small_case():
    return dict(C.tail_cases()[0])


@pytest.mark.parametrize("what,field,value", [("F = 17", "num_filters", 17), ("width 25", "param_width", 25),
                                              ("forced_id = F", "forced_id", None), ("noise_stride 0", "noise_stride", 0)])
def test_tail_refuses_what_it_cannot_run(L, what, field, value):
    from adaptiveisp_amd import _lib
    from adaptiveisp_amd.policy_train import _TailArgs
    case = _small_case()
    B, F, pw = case["B"], 17, 25                                             # buffers for the largest reading of the shape
    with torch.cuda.device(DEV):
        a, ins = _TailArgs(), {}
        _shared(a, case, "sample", ins)
        z = torch.zeros(B * F * pw + 64, dtype=torch.float32, device=DEV)
        a.B, a.x, a.logits, a.noise, a.states = B, z.data_ptr(), z.data_ptr(), z.data_ptr(), z.data_ptr()
        outs = {k: _Guarded((B * F * pw,), np.int64 if k == "selected" else np.float32)
                for k in ("table", "packed", "op_ids", "selected", "pdf", "surrogate", "new_states", "penalty", "d_x", "d_logits")}
        for k, o in outs.items():
            setattr(a, k, o.ptr)
        setattr(a, field, case["F"] if value is None else value)
        rcs = (L.adaisp_policy_tail_fwd(ctypes.byref(a), _lib._stream()), L.adaisp_policy_tail_bwd(ctypes.byref(a), _lib._stream()))
        torch.cuda.synchronize()
    assert rcs == (ESHAPE, ESHAPE), f"{what}: returned {rcs}"
    assert all(o.untouched() for o in outs.values())


@pytest.mark.parametrize("what,field,value", [("F = 17", "num_filters", 17), ("width 25", "param_width", 25),
                                              ("forced_id = F", "forced_id", None), ("noise_stride 0", "noise_stride", 0)])
def test_finish_refuses_what_it_cannot_run(L, what, field, value):
    from adaptiveisp_amd import _lib
    from adaptiveisp_amd.policy_fast import _FinishArgs
    case = dict(C.finish_cases()[1])
    B, F, pw = case["B"], 17, 25
    with torch.cuda.device(DEV):
        a, ins = _FinishArgs(), {}
        _shared(a, case, "train_mode", ins)
        z = torch.zeros((F + 1) * case["hid"] * pw + 64, dtype=torch.float32, device=DEV)
        zi = torch.zeros(F * pw, dtype=torch.int32, device=DEV)
        for k in ("hidden", "w_filter", "b_filter", "w_sel", "b_sel", "noise", "states"):
            setattr(a, k, z.data_ptr())
        a.row_filter, a.row_slot, a.num_rows, a.hid = zi.data_ptr(), zi.data_ptr(), case["row_filter"].size, case["hid"]
        outs = {k: _Guarded((B * F * pw,), np.int64 if k == "selected" else np.float32)
                for k in ("params_all", "packed", "op_ids", "selected", "pdf_out", "surrogate", "new_states", "penalty")}
        for k, o in outs.items():
            setattr(a, k, o.ptr)
        setattr(a, field, case["F"] if value is None else value)
        rc = L.adaisp_policy_finish(ctypes.byref(a), B, _lib._stream())
        torch.cuda.synchronize()
    assert rc == ESHAPE, f"{what}: returned {rc}"
    assert all(o.untouched() for o in outs.values())
