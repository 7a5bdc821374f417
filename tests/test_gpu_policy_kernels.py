"""The eval policy step's trunk and fc1 kernels (csrc/isp_policy.hip: k_trunk_mfma, k_trunk_conv, k_fc1) through the C ABI
(adaisp_policy_conv, adaisp_policy_fc1), one layer at a time, against the float64 restatements of tests/_policyref.py (pinned to
the PyTorch modules by tests/test_policyref_host.py).

Three kinds of check per shape:
  exact    inputs on power-of-two lattices: every product is a multiple of 2^-10 and every partial sum stays below 2^11, so the
           fp32 pre-activation is exact in any summation order and the output must equal the float64 result bit for bit
           (a dropped tap, a swapped channel, a wrong pad, a slice boundary off by one, a lost split-K partial: all fail);
  bounded  random data against the any-order summation bound  |got - ref| <= (K + KS + 2) u A + u |ref|,  u = 2^-24,
           A = sum |in| |w| + |bias|: K products and K + KS - 1 additions can sit on no chain longer than K + KS, the bias add
           and the 0.2 multiply round once each; KS <= 16 slices, 16 is used. (The reference multiplies by the double 0.2, the
           kernel by 0.2f = 0.2 (1 + u / 4): that is u |ref| / 4 on outputs whose summation error the multiply has just cut to
           a fifth, far inside the first term.) Reduced-precision products or accumulation, which the lattice cannot see, fail;
  repeat   the same launch three times gives the same bits (fixed summation order).
Every output buffer sits between NaN-filled guards that must stay NaN, and must itself come back without a NaN."""
import ctypes

import numpy as np
import pytest
import torch

import _policyref as R
from _margins import close

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
GUARD = 256                     # floats before and after every output
U = 2.0 ** -24
KS_MAX = 16
ESHAPE = -4                     # ADAISP_ESHAPE (include/adaisp.h)


def _mfma_form(Cin, Cout):
    """launch_policy_conv's rule: the matrix-core form takes these shapes, k_trunk_conv the rest."""
    return Cin % 8 == 0 and Cout % 16 == 0


# (G, B, Cin, Hin, Cout, states?)
PRODUCTION = [(2, B, *layer) for B in (1, 3, 8, 9)
              for layer in ((16, 64, 32, True), (32, 32, 64, False), (64, 16, 128, False), (128, 8, 256, False))]
MFMA_EDGES = [(1, 1, 8, 4, 16, False),        # KS = 1 (no LDS), npix = 4: twelve dead columns
              (1, 3, 8, 4, 16, True),         # n_state = 5
              (3, 5, 24, 2, 48, False),       # KS = 3, Ho = 1, npix = 5
              (1, 3, 128, 4, 16, False),      # KS = 16, partial tile
              (2, 2, 16, 8, 48, True)]
FALLBACK = [(2, 3, 15, 8, 32, True),          # a 9-filter list: n_state = 12; 48 pixels in a 64-pixel tile
            (1, 2, 3, 8, 8, True),            # n_state = 0
            (1, 1, 5, 4, 8, False),           # odd Cin: the two-channel trip's tail
            (2, 4, 20, 8, 24, False),         # KS = 2
            (1, 2, 100, 4, 8, False),         # KS = 12, odd slice width
            (1, 1, 121, 4, 16, False),        # KS = 15, the last slice is empty
            (1, 5, 127, 4, 8, False),
            (2, 3, 128, 4, 40, False)]        # Cout % 16 == 8, KS = 16, exactly 64 KB of LDS
CONV_CASES = [(c, True) for c in PRODUCTION + MFMA_EDGES] + [(c, False) for c in FALLBACK]
FC1_CASES = [(B, 4096, 11, 128) for B in (1, 3, 8, 9, 17)] + [(3, 1024, 1, 4), (9, 2048, 3, 132)]      # (B, D, NH, HID)


def _id(v):
    return "-".join(str(int(x)) for x in v[0]) + ("-mfma" if v[1] else "-fallback") if isinstance(v[0], tuple) else \
        "-".join(str(int(x)) for x in v)


@pytest.fixture(scope="module")
def L():
    from adaptiveisp_amd import _lib
    lib = _lib.load()
    vp, ci = ctypes.c_void_p, ctypes.c_int
    lib.adaisp_policy_conv.argtypes = [vp, vp, ci, vp, vp, vp, ci, ci, ci, ci, ci, vp]
    lib.adaisp_policy_fc1.argtypes = [vp, vp, vp, vp, vp, ci, ci, ci, ci, vp]
    lib.adaisp_policy_conv.restype = lib.adaisp_policy_fc1.restype = ci
    return lib


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


class _Guarded:
    """n output floats between two NaN-filled guards; the output itself starts as NaN too."""

    def __init__(self, n):
        self.n = n
        self.buf = torch.full((GUARD + n + GUARD,), float("nan"), dtype=torch.float32, device=DEV)
        self.ptr = self.buf.data_ptr() + 4 * GUARD

    def read(self, what):
        h = self.buf.cpu().numpy()
        assert np.isnan(h[:GUARD]).all() and np.isnan(h[GUARD + self.n:]).all(), f"{what}: wrote outside its output"
        out = h[GUARD:GUARD + self.n].copy()
        assert not np.isnan(out).any(), f"{what}: {int(np.isnan(out).sum())} of {self.n} outputs not written (or NaN)"
        return out

    def untouched(self):
        return bool(torch.isnan(self.buf).all())


def _conv(L, case, inp, states, w, bias, launches=1):
    from adaptiveisp_amd import _lib
    G, B, Cin, Hin, Cout, has_states = case
    Ho = Hin // 2
    d_in, d_w, d_b = _dev(inp), _dev(w), _dev(bias)
    d_st = _dev(states if states.size else np.zeros(1, np.float32)) if has_states else None      # n_state = 0: still a pointer
    outs = []
    with torch.cuda.device(DEV):
        for _ in range(launches):
            o = _Guarded(G * B * Cout * Ho * Ho)
            rc = L.adaisp_policy_conv(d_in.data_ptr(), d_st.data_ptr() if has_states else None, Cin - 3 if has_states else 0,
                                      d_w.data_ptr(), d_b.data_ptr(), o.ptr, G, B, Cin, Hin, Cout, _lib._stream())
            _lib._check(rc, "adaisp_policy_conv")
            torch.cuda.synchronize()
            outs.append(o.read(f"adaisp_policy_conv{case}").reshape(G, B, Cout, Ho, Ho))
    return outs[0] if launches == 1 else outs


def _fc1(L, case, feats, src, w1, b1, launches=1):
    from adaptiveisp_amd import _lib
    B, D, NH, HID = case
    d = [_dev(a) for a in (feats, src, w1, b1)]
    outs = []
    with torch.cuda.device(DEV):
        for _ in range(launches):
            o = _Guarded(B * NH * HID)
            rc = L.adaisp_policy_fc1(*[t.data_ptr() for t in d], o.ptr, B, D, NH, HID, _lib._stream())
            _lib._check(rc, "adaisp_policy_fc1")
            torch.cuda.synchronize()
            outs.append(o.read(f"adaisp_policy_fc1{case}").reshape(B, NH, HID))
    return outs[0] if launches == 1 else outs


def _conv_inputs(case, rng, kind):
    """kind 'lattice' | 'unit' (inputs uniform in [0, 1]: images, states, LeakyReLU outputs) | 'signed'."""
    G, B, Cin, Hin, Cout, has_states = case
    K = 16 * Cin
    ishape = (B, 3, Hin, Hin) if has_states else (G, B, Cin, Hin, Hin)
    sshape = (B, Cin - 3) if has_states else (0,)
    if kind == "lattice":
        inp, st = R.lattice(rng, ishape, 1 / 16, 1.0, signed=False), R.lattice(rng, sshape, 1 / 16, 1.0, signed=False)
        w, bias = R.lattice(rng, (G, Cout, Cin, 4, 4), 1 / 64, 1.0), R.lattice(rng, (G, Cout), 2.0 ** -10, 1.0)
    else:
        lo = 0.0 if kind == "unit" else -1.0
        inp, st = (rng.uniform(lo, 1.0, s).astype(np.float32) for s in (ishape, sshape))
        w = (rng.normal(size=(G, Cout, Cin, 4, 4)) / np.sqrt(K)).astype(np.float32)
        bias = rng.normal(0.0, 0.3, (G, Cout)).astype(np.float32)
    return inp, st, w, bias


def _fc1_inputs(case, rng, kind):
    B, D, NH, HID = case
    src = np.array([1 if h % 3 == 0 else 0 for h in range(NH)], dtype=np.int32)      # both trunks wherever NH allows
    if kind == "lattice":
        feats = R.lattice(rng, (2, B, D), 1 / 16, 1.0)
        w1, b1 = R.lattice(rng, (NH, HID, D), 1 / 64, 0.5), R.lattice(rng, (NH, HID), 2.0 ** -10, 1.0)
    else:
        feats = rng.uniform(0.0 if kind == "unit" else -1.0, 1.0, (2, B, D)).astype(np.float32)
        w1 = (rng.normal(size=(NH, HID, D)) / np.sqrt(D)).astype(np.float32)
        b1 = rng.normal(0.0, 0.3, (NH, HID)).astype(np.float32)
    return feats, src, w1, b1


def _exact(got, pre64, what):
    pre32 = pre64.astype(np.float32)
    assert np.array_equal(pre32.astype(np.float64), pre64), "the lattice sum is not a float32: test data out of range"
    want = R.lrelu(pre32)                                                    # float32: v > 0 ? v : 0.2f * v
    assert (pre32 < 0).any() and (pre32 > 0).any()
    bad = np.argwhere(got != want)
    assert bad.size == 0, (f"{what}: {len(bad)} of {got.size} outputs differ from the exact result, first at {tuple(bad[0])}: "
                           f"got {got[tuple(bad[0])]!r}, want {want[tuple(bad[0])]!r}")


def _bounded(label, got, ref, A, K, what):
    err = np.abs(got.astype(np.float64) - ref)
    bound = (K + KS_MAX + 2) * U * A + U * np.abs(ref)
    with np.errstate(divide="ignore", invalid="ignore"):
        share = np.where(err == 0, 0.0, err / bound)
    print(f"{what}: largest share of the summation bound used {share.max():.4f} (max abs err {err.max():.3e})")
    close(label, share, np.zeros_like(share), rtol=0, atol=1.0, err_msg=what)


@pytest.mark.parametrize("case,mfma", CONV_CASES, ids=[_id(c) for c in CONV_CASES])
def test_trunk_conv_exact_on_lattice(L, case, mfma):
    assert _mfma_form(case[2], case[4]) == mfma, f"{case} no longer takes the {'matrix-core' if mfma else 'fallback'} form"
    rng = np.random.default_rng([1, *case[:5]])
    inp, st, w, bias = _conv_inputs(case, rng, "lattice")
    pre, _ = R.trunk_conv(inp, st if case[5] else None, w, bias, act=False)
    _exact(_conv(L, case, inp, st, w, bias), pre, f"adaisp_policy_conv{case}")


@pytest.mark.parametrize("case,mfma", CONV_CASES, ids=[_id(c) for c in CONV_CASES])
def test_trunk_conv_within_summation_bound(L, case, mfma):
    assert _mfma_form(case[2], case[4]) == mfma, f"{case} no longer takes the {'matrix-core' if mfma else 'fallback'} form"
    rng = np.random.default_rng([2, *case[:5]])
    for kind in ("unit", "signed"):
        inp, st, w, bias = _conv_inputs(case, rng, kind)
        ref, A = R.trunk_conv(inp, st if case[5] else None, w, bias)
        _bounded("policy.trunk_mfma" if mfma else "policy.trunk_conv", _conv(L, case, inp, st, w, bias), ref, A, 16 * case[2],
                 f"adaisp_policy_conv{case} {kind}")


@pytest.mark.parametrize("case", FC1_CASES, ids=[_id(c) for c in FC1_CASES])
def test_fc1_exact_on_lattice(L, case):
    rng = np.random.default_rng([3, *case])
    feats, src, w1, b1 = _fc1_inputs(case, rng, "lattice")
    assert case[2] == 1 or set(src.tolist()) == {0, 1}
    pre, _ = R.fc1(feats, src, w1, b1, act=False)
    _exact(_fc1(L, case, feats, src, w1, b1), pre, f"adaisp_policy_fc1{case}")


@pytest.mark.parametrize("case", FC1_CASES, ids=[_id(c) for c in FC1_CASES])
def test_fc1_within_summation_bound(L, case):
    rng = np.random.default_rng([4, *case])
    for kind in ("unit", "signed"):
        feats, src, w1, b1 = _fc1_inputs(case, rng, kind)
        ref, A = R.fc1(feats, src, w1, b1)
        _bounded("policy.fc1", _fc1(L, case, feats, src, w1, b1), ref, A, case[1], f"adaisp_policy_fc1{case} {kind}")


def test_trunk_mfma_split_k_repeats_bit_for_bit(L):
    case = (2, 9, 128, 8, 256, False)                                        # KS = 16 waves meet in LDS
    assert _mfma_form(case[2], case[4])
    a, b, c = _conv(L, case, *_conv_inputs(case, np.random.default_rng(5), "signed"), launches=3)
    assert np.array_equal(a.view(np.int32), b.view(np.int32)) and np.array_equal(a.view(np.int32), c.view(np.int32))


def test_fc1_repeats_bit_for_bit(L):
    case = (9, 4096, 11, 128)                                                # two trips of the batch loop
    a, b, c = _fc1(L, case, *_fc1_inputs(case, np.random.default_rng(6), "signed"), launches=3)
    assert np.array_equal(a.view(np.int32), b.view(np.int32)) and np.array_equal(a.view(np.int32), c.view(np.int32))


@pytest.mark.parametrize("what,Cin,Hin,Cout,n_state", [("Cin", 136, 8, 16, None), ("Cout", 16, 8, 12, None),
                                                       ("Hin", 16, 7, 16, None), ("n_state", 16, 8, 16, 12)])
def test_conv_refuses_shapes_it_cannot_run(L, what, Cin, Hin, Cout, n_state):
    from adaptiveisp_amd import _lib
    G, B = 1, 2
    z = lambda n: torch.zeros(n, dtype=torch.float32, device=DEV)  # noqa: E731
    d_in, d_w, d_b, d_st = z(G * B * Cin * Hin * Hin), z(G * Cout * Cin * 16), z(G * Cout), z(B * 16)
    o = _Guarded(G * B * Cout * Hin * Hin)                                   # more than any reading of the shape would write
    with torch.cuda.device(DEV):
        rc = L.adaisp_policy_conv(d_in.data_ptr(), d_st.data_ptr() if n_state is not None else None, n_state or 0, d_w.data_ptr(),
                                  d_b.data_ptr(), o.ptr, G, B, Cin, Hin, Cout, _lib._stream())
        torch.cuda.synchronize()
    assert rc == ESHAPE, f"bad {what}: returned {rc}"
    assert o.untouched()


@pytest.mark.parametrize("D,HID", [(1000, 8), (1024, 6)])
def test_fc1_refuses_shapes_it_cannot_run(L, D, HID):
    from adaptiveisp_amd import _lib
    B, NH = 2, 2
    d_f = torch.zeros(2 * B * D, dtype=torch.float32, device=DEV)
    d_src = torch.zeros(NH, dtype=torch.int32, device=DEV)
    d_w, d_b = torch.zeros(NH * HID * D, dtype=torch.float32, device=DEV), torch.zeros(NH * HID, dtype=torch.float32, device=DEV)
    o = _Guarded(B * NH * HID)
    with torch.cuda.device(DEV):
        rc = L.adaisp_policy_fc1(d_f.data_ptr(), d_src.data_ptr(), d_w.data_ptr(), d_b.data_ptr(), o.ptr, B, D, NH, HID,
                                 _lib._stream())
        torch.cuda.synchronize()
    assert rc == ESHAPE, f"D={D} HID={HID}: returned {rc}"
    assert o.untouched()
