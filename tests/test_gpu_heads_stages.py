"""The six training heads kernels (csrc/isp_heads_train.hip: k_heads_fc1, k_heads_out, k_heads_dhid, k_heads_dw1,
k_heads_dfeat_part, k_heads_dfeat_sum) through adaisp_heads_fwd / _bwd, stage by stage against the float64 restatements of
tests/_tailref.py, at the limits heads_check admits: hid 8 to 256, D = 1024, F = 1 and 16, width 24, F > width, B = 1 to 8.

Each stage is compared on the device's OWN upstream buffers (`hidden` and `dhid` are caller-visible), so every sum is one short
dot product with the any-order bound |got - ref| <= (K + 2) u A + u |ref|, u = 2^-24, A = sum |products| + |bias| and K the
longest chain of additions; LeakyReLU's slope is decided by the sign of the device's `hidden`, so nothing is ambiguous. One
end-to-end comparison with float64 autograd (1e-5 of each tensor's scale, the project's cap for fp32 arithmetic, not a device
measurement) confirms that the stages are chained correctly. k_heads_fc1 also runs a lattice case that must match bit for bit.
Every output and scratch buffer sits between NaN guards, and two runs give the same bits."""
import ctypes

import numpy as np
import pytest
import torch

import _policyref as P
import _tailref as R
from _margins import close, close_scaled

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
GUARD = 256
U = 2.0 ** -24
ESHAPE = -4

# (B, F, D, hid, pw, n)
SHAPES = [(8, 10, 4096, 128, 9, [1, 1, 9, 1, 1, 8, 1, 1, 1, 3]), (1, 10, 4096, 128, 9, [1, 1, 9, 1, 1, 8, 1, 1, 1, 3]),
          (3, 10, 4096, 128, 9, [1, 1, 9, 1, 1, 8, 1, 1, 1, 3]), (5, 1, 1024, 8, 1, [1]), (8, 16, 1024, 256, 24, [24] * 16),
          (3, 2, 2048, 72, 24, [24, 1]), (2, 16, 1024, 64, 3, [3, 1, 2, 3, 1, 1, 2, 3, 3, 1, 2, 1, 3, 2, 1, 3])]   # F > width sizes the LDS
IDS = ["-".join(str(v) for v in s[:5]) for s in SHAPES]


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


class _Guarded:
    def __init__(self, shape):
        self.shape, self.n = tuple(shape), int(np.prod(shape))
        self.buf = torch.full((GUARD + self.n + GUARD,), float("nan"), dtype=torch.float32, device=DEV)
        self.ptr = self.buf.data_ptr() + 4 * GUARD

    def read(self, what):
        h = self.buf.cpu().numpy()
        assert np.isnan(h[:GUARD]).all() and np.isnan(h[GUARD + self.n:]).all(), f"{what}: wrote outside its buffer"
        out = h[GUARD:GUARD + self.n].copy()
        assert not np.isnan(out).any(), f"{what}: {int(np.isnan(out).sum())} of {self.n} values not written (or NaN)"
        return out.reshape(self.shape)

    def untouched(self):
        return bool(torch.isnan(self.buf).all())


def _inputs(shape, rng, lattice=False):
    B, F, D, hid, pw, n = shape
    if lattice:
        f = lambda *s: P.lattice(rng, s, 2.0 ** -3, 1.0)  # noqa: E731
        w = lambda *s: P.lattice(rng, s, 2.0 ** -5, 2.0 ** -2)  # noqa: E731
        b = lambda *s: P.lattice(rng, s, 2.0 ** -8, 1.0)  # noqa: E731
    else:
        f = lambda *s: rng.normal(size=s).astype(np.float32)  # noqa: E731
        w = lambda *s: (rng.normal(size=s) / np.sqrt(s[-1])).astype(np.float32)  # noqa: E731
        b = lambda *s: rng.normal(0.0, 0.3, s).astype(np.float32)  # noqa: E731
    g = lambda *s: rng.normal(size=s).astype(np.float32)  # noqa: E731
    return dict(feat_f=f(B, D), feat_s=f(B, D), w1=[w(hid, D) for _ in n], b1=[b(hid) for _ in n], wf=[w(k, hid) for k in n],
                bf=[b(k) for k in n], ws1=w(hid, D), bs1=b(hid), ws2=w(F, hid), bs2=b(F), dx=g(B, F, pw), dlogits=g(B, F))


def _run(L, shape, t, backward=True):
    """adaisp_heads_fwd (and _bwd) on guarded buffers -> dict of host arrays."""
    from adaptiveisp_amd import _lib
    from adaptiveisp_amd.heads_train import _HeadsArgs
    B, F, D, hid, pw, n = shape
    a = _HeadsArgs()
    a.B, a.F, a.D, a.hid, a.pw = B, F, D, hid, pw
    d = {k: ([_dev(v) for v in t[k]] if isinstance(t[k], list) else _dev(t[k])) for k in t}
    for j in range(F):
        a.n[j] = n[j]
        a.w1[j], a.b1[j], a.wf[j], a.bf[j] = (d[k][j].data_ptr() for k in ("w1", "b1", "wf", "bf"))
    for k in ("feat_f", "feat_s", "ws1", "bs1", "ws2", "bs2", "dx", "dlogits"):
        setattr(a, k, d[k].data_ptr())
    G = F + 1
    o = dict(hidden=_Guarded((B, G, hid)), x=_Guarded((B, F, pw)), logits=_Guarded((B, F)))
    if backward:
        o.update(dhid=_Guarded((B, G, hid)), part=_Guarded((G, B, D)), dws1=_Guarded((hid, D)), dbs1=_Guarded((hid,)),
                 dws2=_Guarded((F, hid)), dbs2=_Guarded((F,)), dfeat_f=_Guarded((B, D)), dfeat_s=_Guarded((B, D)))
        for j in range(F):
            o.update({f"dw1.{j}": _Guarded((hid, D)), f"db1.{j}": _Guarded((hid,)), f"dwf.{j}": _Guarded((n[j], hid)),
                      f"dbf.{j}": _Guarded((n[j],))})
            a.dw1[j], a.db1[j], a.dwf[j], a.dbf[j] = (o[f"{k}.{j}"].ptr for k in ("dw1", "db1", "dwf", "dbf"))
    for k, v in o.items():
        if "." not in k:
            setattr(a, k, v.ptr)
    with torch.cuda.device(DEV):
        _lib._check(L.adaisp_heads_fwd(ctypes.byref(a), _lib._stream()), "adaisp_heads_fwd")
        if backward:
            _lib._check(L.adaisp_heads_bwd(ctypes.byref(a), _lib._stream()), "adaisp_heads_bwd")
        torch.cuda.synchronize()
    return {k: v.read(f"adaisp_heads {shape[:5]} {k}") for k, v in o.items()}


@pytest.fixture(scope="module")
def L():
    from adaptiveisp_amd import _lib
    from adaptiveisp_amd.heads_train import _HeadsArgs
    lib = _lib.load()
    lib.adaisp_heads_fwd.argtypes = lib.adaisp_heads_bwd.argtypes = [ctypes.POINTER(_HeadsArgs), ctypes.c_void_p]
    lib.adaisp_heads_fwd.restype = lib.adaisp_heads_bwd.restype = ctypes.c_int
    yield lib
    _RUNS.clear()                                                            # the shapes' host copies go with the module


_RUNS = {}


def _device_run(L, i):
    """Inputs and two device runs of shape i, made once and shared by the tests of that shape."""
    if i not in _RUNS:
        t = _inputs(SHAPES[i], np.random.default_rng([7, i]))
        _RUNS[i] = (t, _run(L, SHAPES[i], t), _run(L, SHAPES[i], t))
    return _RUNS[i]


def _bounded(label, got, ref, A, K, what):
    err = np.abs(np.asarray(got, dtype=np.float64) - ref)
    bound = (np.asarray(K, dtype=np.float64) + 2) * U * A + U * np.abs(ref)
    with np.errstate(divide="ignore", invalid="ignore"):
        share = np.where(err == 0, 0.0, err / bound)
    print(f"{what} {label}: largest share of the summation bound used {share.max():.4f} (max abs err {err.max():.3e})")
    close(label, share, np.zeros_like(share), rtol=0, atol=1.0, err_msg=what)


@pytest.mark.parametrize("i", range(len(SHAPES)), ids=IDS)
def test_repeat_runs_give_equal_bits(L, i):
    _, a, b = _device_run(L, i)
    assert a.keys() == b.keys()
    for k in a:
        assert np.array_equal(a[k].view(np.int32), b[k].view(np.int32)), f"{SHAPES[i][:5]}: {k} differs between two runs"


@pytest.mark.parametrize("i", range(len(SHAPES)), ids=IDS)
def test_forward_stages_within_summation_bound(L, i):
    shape = SHAPES[i]
    B, F, D, hid, pw, n = shape
    t, got, _ = _device_run(L, i)
    ref, A = R.heads_fc1(t["feat_f"], t["feat_s"], t["w1"], t["b1"], t["ws1"], t["bs1"])
    _bounded("heads.fc1", got["hidden"], ref, A, D, f"{shape[:5]}")
    assert (got["hidden"] > 0).any() and (got["hidden"] < 0).any()
    x, Ax, lg, Al = R.heads_out(got["hidden"], t["wf"], t["bf"], t["ws2"], t["bs2"], pw)       # from the device's own hidden
    for f in range(F):
        assert not got["x"][:, f, n[f]:].view(np.uint32).any(), f"{shape[:5]}: x[:, {f}, {n[f]}:] is not +0"
        _bounded("heads.out.x", got["x"][:, f, :n[f]], x[:, f, :n[f]], Ax[:, f, :n[f]], hid, f"{shape[:5]} filter {f}")
    _bounded("heads.out.logits", got["logits"], lg, Al, hid, f"{shape[:5]}")


@pytest.mark.parametrize("i", range(len(SHAPES)), ids=IDS)
def test_backward_stages_within_summation_bound(L, i):
    shape = SHAPES[i]
    B, F, D, hid, pw, n = shape
    t, got, _ = _device_run(L, i)
    what = f"{shape[:5]}"
    dhid, Ad = R.heads_dhid(got["hidden"], t["dx"], t["dlogits"], t["wf"], t["ws2"])
    K = np.array(n + [F], dtype=np.float64)[None, :, None]                   # rows of each group
    _bounded("heads.dhid", got["dhid"], dhid, Ad, K, what)
    for g, (dW, AW, db, Ab) in enumerate(R.heads_dw2(got["hidden"], t["dx"], t["dlogits"], n)):
        kw, kb = ("dws2", "dbs2") if g == F else (f"dwf.{g}", f"dbf.{g}")
        _bounded("heads.dw2", got[kw], dW, AW, B, f"{what} group {g}")
        _bounded("heads.db2", got[kb], db, Ab, B, f"{what} group {g}")
    dW1, AW1, db1, Ab1 = R.heads_dw1(got["dhid"], t["feat_f"], t["feat_s"])                # from the device's own dhid
    for g in range(F + 1):
        kw, kb = ("dws1", "dbs1") if g == F else (f"dw1.{g}", f"db1.{g}")
        _bounded("heads.dw1", got[kw], dW1[g], AW1[g], B, f"{what} group {g}")
        _bounded("heads.db1", got[kb], db1[g], Ab1[g], B, f"{what} group {g}")
    dff, Af, dfs, As = R.heads_dfeat(got["dhid"], t["w1"], t["ws1"])
    _bounded("heads.dfeat_f", got["dfeat_f"], dff, Af, hid + F, what)
    _bounded("heads.dfeat_s", got["dfeat_s"], dfs, As, hid, what)


@pytest.mark.parametrize("i", range(len(SHAPES)), ids=IDS)
def test_fc1_exact_on_lattice(L, i):
    shape = SHAPES[i]
    t = _inputs(shape, np.random.default_rng([8, i]), lattice=True)
    got = _run(L, shape, t, backward=False)["hidden"]
    pre64, A = R.heads_fc1(t["feat_f"], t["feat_s"], t["w1"], t["b1"], t["ws1"], t["bs1"])
    want = pre64.astype(np.float32)
    assert np.array_equal(want.astype(np.float64), pre64) and A.max() < 2.0 ** 11, "the lattice sum is not a float32"
    bad = np.argwhere(got != want)
    assert bad.size == 0, (f"{shape[:5]}: {len(bad)} of {got.size} pre-activations differ from the exact result, first at "
                           f"{tuple(bad[0])}: got {got[tuple(bad[0])]!r}, want {want[tuple(bad[0])]!r}")


@pytest.mark.parametrize("i", range(len(SHAPES)), ids=IDS)
def test_all_gradients_against_float64_autograd(L, i):
    shape = SHAPES[i]
    B, F, D, hid, pw, n = shape
    t, got, _ = _device_run(L, i)
    leaf = lambda a: torch.from_numpy(np.asarray(a, dtype=np.float64)).requires_grad_(True)  # noqa: E731
    p = {k: ([leaf(v) for v in t[k]] if isinstance(t[k], list) else leaf(t[k])) for k in t if k not in ("dx", "dlogits")}
    lin, act = torch.nn.functional.linear, lambda v: torch.nn.functional.leaky_relu(v, 0.2)  # noqa: E731
    x = torch.stack([torch.nn.functional.pad(lin(act(lin(p["feat_f"], p["w1"][g], p["b1"][g])), p["wf"][g], p["bf"][g]),
                                             (0, pw - n[g])) for g in range(F)], dim=1)
    logits = lin(act(lin(p["feat_s"], p["ws1"], p["bs1"])), p["ws2"], p["bs2"])
    names = ["feat_f", "feat_s", "ws1", "bs1", "ws2", "bs2"] + [f"{k}.{g}" for k in ("w1", "b1", "wf", "bf") for g in range(F)]
    leaves = [p[k] for k in names[:6]] + [p[k][g] for k in ("w1", "b1", "wf", "bf") for g in range(F)]
    loss = (x * torch.from_numpy(t["dx"].astype(np.float64))).sum() + (logits * torch.from_numpy(t["dlogits"].astype(np.float64))).sum()
    grads = torch.autograd.grad(loss, leaves)
    close_scaled("heads.chain.x", got["x"], x.detach(), 1e-5, err_msg=str(shape[:5]))
    close_scaled("heads.chain.logits", got["logits"], logits.detach(), 1e-5, err_msg=str(shape[:5]))
    for name, g in zip(names, grads):
        key = {"feat_f": "dfeat_f", "feat_s": "dfeat_s"}.get(name, "d" + name)
        close_scaled("heads.chain." + key.split(".")[0], got[key], g, 1e-5, floor=0.0, err_msg=f"{shape[:5]} {name}")


REFUSED = [("B = 9", dict(B=9)), ("hid = 264", dict(hid=264)), ("hid = 12", dict(hid=12)), ("D = 1000", dict(D=1000)),
           ("n_f = 0", dict(n0=0)), ("n_f > pw", dict(n0=2, pw=1))]


@pytest.mark.parametrize("what,change", REFUSED, ids=[r[0].replace(" ", "") for r in REFUSED])
def test_heads_refuse_what_they_cannot_run(L, what, change):
    from adaptiveisp_amd import _lib
    from adaptiveisp_amd.heads_train import _HeadsArgs
    B, F, D, hid, pw = 9, 1, 1024, 264, 2                                    # buffers for the largest reading of any variant
    z = torch.zeros(hid * D, dtype=torch.float32, device=DEV)
    a = _HeadsArgs()
    a.B, a.F, a.D, a.hid, a.pw = 5, 1, 1024, 8, 2
    a.n[0] = 1
    for k in ("feat_f", "feat_s", "ws1", "bs1", "ws2", "bs2", "dx", "dlogits"):
        setattr(a, k, z.data_ptr())
    a.w1[0] = a.b1[0] = a.wf[0] = a.bf[0] = z.data_ptr()
    sizes = dict(hidden=B * 2 * hid, x=B * F * pw, logits=B * F, dhid=B * 2 * hid, part=2 * B * D, dws1=hid * D, dbs1=hid,
                 dws2=F * hid, dbs2=F, dfeat_f=B * D, dfeat_s=B * D, dw1=hid * D, db1=hid, dwf=pw * hid, dbf=pw)
    o = {k: _Guarded((v,)) for k, v in sizes.items()}
    for k, v in o.items():
        if k in ("dw1", "db1", "dwf", "dbf"):
            getattr(a, k)[0] = v.ptr
        else:
            setattr(a, k, v.ptr)
    for k, v in change.items():
        if k == "n0":
            a.n[0] = v
        else:
            setattr(a, k, v)
    with torch.cuda.device(DEV):
        rcs = (L.adaisp_heads_fwd(ctypes.byref(a), _lib._stream()), L.adaisp_heads_bwd(ctypes.byref(a), _lib._stream()))
        torch.cuda.synchronize()
    assert rcs == (ESHAPE, ESHAPE), f"{what}: returned {rcs}"
    assert all(v.untouched() for v in o.values())
