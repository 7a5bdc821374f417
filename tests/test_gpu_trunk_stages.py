"""The training-mode trunk kernels (csrc/isp_trunk_train.hip: k_tconv_fwd, k_tbn_fwd, k_tbn_bwd, k_twgrad, k_twgrad_reduce,
k_tdgrad, k_tplane_sum) through adaisp_trunk_train_fwd / _bwd, stage by stage against the float64 restatements of
tests/_trunkref.py, on the cases of _trunkref.CASES: the smallest shapes that reach every launch geometry the host code picks
from B and C.

Each stage is compared on the device's OWN upstream buffers, read out of the workspace and the scratch through _trunkref.plan
(whose totals must equal adaisp_trunk_train_workspace_bytes / _scratch_bytes), with the LeakyReLU branch of the backward
decided by the device's own activation. Every bound is derived from u = 2^-24, the length K of the kernel's longest chain of
additions for that geometry and the magnitude sum A (_trunkref.stage_shares states each derivation); none comes from a
device measurement. tests/test_trunkref_host.py shows that float32 arithmetic in two summation orders uses at most a quarter
of every bound, and that eleven deliberate errors break one. The share of each bound the device uses is recorded under the
`trunk_stages.*` labels.

Chain check, B <= 33 only: features, running statistics, every gradient and the input gradients against _trunkref.chain in
float64, masks from the device's activations, as a fraction of each tensor's scale: _trunkref.CHAIN_FRAC, 4x the largest
fraction the float32 restatements reach on those cases on the host (measured there, rounded up: features 2.1e-6, running statistics
3.1e-7, gradients 3.2e-6, input gradients 1.1e-6, so the bounds are 8.4e-6, 1.24e-6, 1.28e-5 and 4.4e-6 of scale), never
looser than today's call-site caps 2e-5 / 1e-5 / 2e-4 / 2e-4. A conv-bias gradient, 0 in exact arithmetic, is held to that
fraction of its layer's weight-gradient scale. The larger batches
(129, 513) get the stage checks only: there float32 and float64 take different LeakyReLU branches at a few of the
2.1 M inputs whose z is within rounding of 0, and float32 sums over 525 312 values of a channel differ from float64 by
2.5e-3 of the input gradient's scale whatever the kernel does, so an end-to-end bound could neither pass reliably nor mean
anything; every stage of those batches is still held to its own bound.

Every output, the workspace and the scratch are NaN-filled between NaN guards: nothing outside is written, every value inside
is (gradients are written, not accumulated into), and two runs give equal bits.

Launch geometry per case and layer (_trunkref.geometry_table(), asserted equal by tests/test_trunkref_host.py):

  b1-two-sets
    L1 bn REG nthr 1024 N 1024 | wgrad PS 1 KS 16 spw 4 U 4 | conv KS 2 cpw 8 pad 0 masked waves 0 | dgrad KS 4 cpw 8
    L2 bn REG nthr 256 N 256 | wgrad PS 1 KS 16 spw 1 U 1 | conv KS 4 cpw 8 pad 0 masked waves 0 | dgrad KS 8 cpw 8
    L3 bn REG nthr 64 N 64 | wgrad PS 1 KS 4 spw 1 U 1 | conv KS 8 cpw 8 pad 0 masked waves 0 | dgrad KS 16 cpw 8
    L4 bn REG nthr 64 N 16 | wgrad PS 1 KS 1 spw 1 U 1 | conv KS 16 cpw 8 pad 0 masked waves 0 | dgrad KS 16 cpw 16
  b3-two-sets
    L1 bn REG nthr 1024 N 3072 | wgrad PS 2 KS 16 spw 6 U 2 | conv KS 2 cpw 8 pad 0 masked waves 0 | dgrad KS 4 cpw 8
    L2 bn REG nthr 768 N 768 | wgrad PS 1 KS 16 spw 3 U 1 | conv KS 4 cpw 8 pad 0 masked waves 0 | dgrad KS 8 cpw 8
    L3 bn REG nthr 192 N 192 | wgrad PS 1 KS 12 spw 1 U 1 | conv KS 8 cpw 8 pad 0 masked waves 0 | dgrad KS 16 cpw 8
    L4 bn REG nthr 64 N 48 | wgrad PS 1 KS 3 spw 1 U 1 | conv KS 16 cpw 8 pad 0 masked waves 0 | dgrad KS 16 cpw 16
  b5-shared
    L1 bn REG nthr 1024 N 5120 | wgrad PS 4 KS 16 spw 5 U 1 | conv KS 3 cpw 8 pad 5 masked waves 0 | dgrad KS 4 cpw 8
    L2 bn REG nthr 1024 N 1280 | wgrad PS 1 KS 16 spw 5 U 1 | conv KS 4 cpw 8 pad 0 masked waves 0 | dgrad KS 8 cpw 8
    L3 bn REG nthr 320 N 320 | wgrad PS 1 KS 10 spw 2 U 2 | conv KS 8 cpw 8 pad 0 masked waves 0 | dgrad KS 16 cpw 8
    L4 bn REG nthr 128 N 80 | wgrad PS 1 KS 5 spw 1 U 1 | conv KS 16 cpw 8 pad 0 masked waves 0 | dgrad KS 16 cpw 16
  b7
    L1 bn REG nthr 1024 N 7168 | wgrad PS 4 KS 16 spw 7 U 1 | conv KS 2 cpw 8 pad 0 masked waves 0 | dgrad KS 4 cpw 8
    L2 bn REG nthr 1024 N 1792 | wgrad PS 1 KS 16 spw 7 U 1 | conv KS 4 cpw 8 pad 0 masked waves 0 | dgrad KS 8 cpw 8
    L3 bn REG nthr 448 N 448 | wgrad PS 1 KS 14 spw 2 U 2 | conv KS 8 cpw 8 pad 0 masked waves 0 | dgrad KS 16 cpw 8
    L4 bn REG nthr 128 N 112 | wgrad PS 1 KS 7 spw 1 U 1 | conv KS 16 cpw 8 pad 0 masked waves 0 | dgrad KS 16 cpw 16
  b8-agent-pair
    L1 bn REG nthr 1024 N 8192 | wgrad PS 8 KS 16 spw 4 U 4 | conv KS 2 cpw 8 pad 0 masked waves 0 | dgrad KS 4 cpw 8
    L2 bn REG nthr 1024 N 2048 | wgrad PS 2 KS 16 spw 4 U 4 | conv KS 4 cpw 8 pad 0 masked waves 0 | dgrad KS 8 cpw 8
    L3 bn REG nthr 512 N 512 | wgrad PS 1 KS 16 spw 2 U 2 | conv KS 8 cpw 8 pad 0 masked waves 0 | dgrad KS 16 cpw 8
    L4 bn REG nthr 128 N 128 | wgrad PS 1 KS 8 spw 1 U 1 | conv KS 16 cpw 8 pad 0 masked waves 0 | dgrad KS 16 cpw 16
  b8-critic-pair
    L1 bn REG nthr 1024 N 8192 | wgrad PS 8 KS 16 spw 4 U 4 | conv KS 3 cpw 8 pad 5 masked waves 0 | dgrad KS 4 cpw 8
    L2 bn REG nthr 1024 N 2048 | wgrad PS 2 KS 16 spw 4 U 4 | conv KS 4 cpw 8 pad 0 masked waves 0 | dgrad KS 8 cpw 8
    L3 bn REG nthr 512 N 512 | wgrad PS 1 KS 16 spw 2 U 2 | conv KS 8 cpw 8 pad 0 masked waves 0 | dgrad KS 16 cpw 8
    L4 bn REG nthr 128 N 128 | wgrad PS 1 KS 8 spw 1 U 1 | conv KS 16 cpw 8 pad 0 masked waves 0 | dgrad KS 16 cpw 16
  b9
    L1 bn STREAM nthr 1024 N 9216 | wgrad PS 8 KS 12 spw 6 U 2 | conv KS 2 cpw 8 pad 0 masked waves 0 | dgrad KS 4 cpw 8
    L2 bn REG nthr 1024 N 2304 | wgrad PS 2 KS 12 spw 6 U 2 | conv KS 4 cpw 8 pad 0 masked waves 0 | dgrad KS 8 cpw 8
    L3 bn REG nthr 576 N 576 | wgrad PS 1 KS 12 spw 3 U 1 | conv KS 8 cpw 8 pad 0 masked waves 0 | dgrad KS 16 cpw 8
    L4 bn REG nthr 192 N 144 | wgrad PS 1 KS 9 spw 1 U 1 | conv KS 16 cpw 8 pad 0 masked waves 0 | dgrad KS 16 cpw 16
  b17-shared
    L1 bn STREAM nthr 1024 N 17408 | wgrad PS 8 KS 8 spw 17 U 1 | conv KS 3 cpw 8 pad 5 masked waves 0 | dgrad KS 4 cpw 8
    L2 bn REG nthr 1024 N 4352 | wgrad PS 4 KS 4 spw 17 U 1 | conv KS 4 cpw 8 pad 0 masked waves 0 | dgrad KS 8 cpw 8
    L3 bn REG nthr 1024 N 1088 | wgrad PS 1 KS 4 spw 17 U 1 | conv KS 8 cpw 8 pad 0 masked waves 0 | dgrad KS 16 cpw 8
    L4 bn REG nthr 320 N 272 | wgrad PS 1 KS 1 spw 17 U 1 | conv KS 16 cpw 8 pad 0 masked waves 0 | dgrad KS 16 cpw 16
  b33
    L1 bn STREAM nthr 1024 N 33792 | wgrad PS 8 KS 12 spw 22 U 2 | conv KS 2 cpw 8 pad 0 masked waves 0 | dgrad KS 4 cpw 8
    L2 bn STREAM nthr 1024 N 8448 | wgrad PS 8 KS 11 spw 6 U 2 | conv KS 4 cpw 8 pad 0 masked waves 0 | dgrad KS 8 cpw 8
    L3 bn REG nthr 1024 N 2112 | wgrad PS 2 KS 11 spw 6 U 2 | conv KS 8 cpw 8 pad 0 masked waves 0 | dgrad KS 16 cpw 8
    L4 bn REG nthr 576 N 528 | wgrad PS 1 KS 11 spw 3 U 1 | conv KS 16 cpw 8 pad 0 masked waves 0 | dgrad KS 16 cpw 16
  b129-narrow
    L1 bn STREAM nthr 1024 N 132096 | wgrad PS 8 KS 12 spw 86 U 2 | conv KS 1 cpw 8 pad 5 masked waves 0 | dgrad KS 2 cpw 8
    L2 bn STREAM nthr 1024 N 33024 | wgrad PS 8 KS 6 spw 43 U 1 | conv KS 2 cpw 8 pad 0 masked waves 0 | dgrad KS 4 cpw 8
    L3 bn STREAM nthr 1024 N 8256 | wgrad PS 4 KS 3 spw 43 U 1 | conv KS 4 cpw 8 pad 0 masked waves 0 | dgrad KS 8 cpw 8
    L4 bn REG nthr 1024 N 2064 | wgrad PS 1 KS 3 spw 43 U 1 | conv KS 8 cpw 8 pad 0 masked waves 0 | dgrad KS 16 cpw 8
  b513-narrow
    L1 bn STREAM nthr 1024 N 525312 | wgrad PS 8 KS 12 spw 342 U 2 | conv KS 1 cpw 8 pad 5 masked waves 0 | dgrad KS 2 cpw 8
    L2 bn STREAM nthr 1024 N 131328 | wgrad PS 8 KS 9 spw 114 U 2 | conv KS 2 cpw 8 pad 0 masked waves 0 | dgrad KS 4 cpw 8
    L3 bn STREAM nthr 1024 N 32832 | wgrad PS 4 KS 9 spw 57 U 1 | conv KS 4 cpw 8 pad 0 masked waves 0 | dgrad KS 8 cpw 8
    L4 bn STREAM nthr 1024 N 8208 | wgrad PS 1 KS 9 spw 57 U 1 | conv KS 8 cpw 8 pad 0 masked waves 0 | dgrad KS 16 cpw 8
  b4-wide
    L1 bn REG nthr 1024 N 4096 | wgrad PS 4 KS 16 spw 4 U 4 | conv KS 3 cpw 8 pad 2 masked waves 0 | dgrad KS 6 cpw 8
    L2 bn REG nthr 1024 N 1024 | wgrad PS 1 KS 16 spw 4 U 4 | conv KS 6 cpw 8 pad 0 masked waves 0 | dgrad KS 12 cpw 8
    L3 bn REG nthr 256 N 256 | wgrad PS 1 KS 16 spw 1 U 1 | conv KS 12 cpw 8 pad 0 masked waves 0 | dgrad KS 12 cpw 16
    L4 bn REG nthr 64 N 64 | wgrad PS 1 KS 4 spw 1 U 1 | conv KS 16 cpw 16 pad 64 masked waves 4 | dgrad KS 16 cpw 24
  b6-sixteen
    L1 bn REG nthr 1024 N 6144 | wgrad PS 4 KS 16 spw 6 U 2 | conv KS 1 cpw 8 pad 5 masked waves 0 | dgrad KS 2 cpw 8
    L2 bn REG nthr 1024 N 1536 | wgrad PS 1 KS 16 spw 6 U 2 | conv KS 2 cpw 8 pad 0 masked waves 0 | dgrad KS 2 cpw 8
    L3 bn REG nthr 384 N 384 | wgrad PS 1 KS 12 spw 2 U 2 | conv KS 2 cpw 8 pad 0 masked waves 0 | dgrad KS 2 cpw 8
    L4 bn REG nthr 128 N 96 | wgrad PS 1 KS 6 spw 1 U 1 | conv KS 2 cpw 8 pad 0 masked waves 0 | dgrad KS 2 cpw 8
"""
import ctypes

import numpy as np
import pytest
import torch

import _trunkref as R
from _margins import close

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
GUARD = 256
EINVAL, ESHAPE = -1, -4
L4 = R.LAYERS


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


class _Guarded:
    """A NaN-filled device buffer between NaN guards; `init` pre-fills the inside (the running statistics are read and written)."""

    def __init__(self, shape, init=None):
        self.shape, self.n = tuple(shape), int(np.prod(shape))
        self.buf = torch.full((GUARD + self.n + GUARD,), float("nan"), dtype=torch.float32, device=DEV)
        if init is not None:
            self.buf[GUARD:GUARD + self.n] = _dev(init).reshape(-1)
        self.ptr = self.buf.data_ptr() + 4 * GUARD

    def raw(self, what):
        h = self.buf.cpu().numpy()
        assert np.isnan(h[:GUARD]).all() and np.isnan(h[GUARD + self.n:]).all(), f"{what}: wrote outside its buffer"
        return h[GUARD:GUARD + self.n]

    def read(self, what):
        out = self.raw(what)
        assert not np.isnan(out).any(), f"{what}: {int(np.isnan(out).sum())} of {self.n} values not written (or NaN)"
        return out.reshape(self.shape)

    def untouched(self):
        return bool(torch.isnan(self.buf).all())


@pytest.fixture(scope="module")
def L():
    from adaptiveisp_amd import _lib
    lib = _lib.load()
    yield lib
    _RUNS.clear()


def _args(c, t, keep):
    """adaisp_trunk_args of a case with the inputs on the device (kept alive in `keep`) and every output in a _Guarded."""
    from adaptiveisp_amd.trunk_train import _Args
    G, B, C, S = c["G"], c["B"], c["C"], c["n_state"]
    a = _Args()
    a.G, a.B, a.n_state, a.share_params = G, B, S, 1 if c["share"] else 0
    for l in range(L4 + 1):
        a.C[l] = C[l]
    a.momentum, a.eps, a.slope = c["momentum"], c["eps"], c["slope"]
    o = {}
    d_img = {id(x): _dev(x) for x in t["img"]}
    d_sv = {id(x): _dev(x) for x in t["svec"] if x is not None}
    d_par = [{k: [_dev(v) for v in p[k]] for k in ("w", "bias", "gamma", "beta")} for p in t["params"]]
    keep += [d_img, d_sv, d_par]
    for s, p in enumerate(t["params"]):
        for l in range(L4):
            o["rmean", l + 1, s] = _Guarded(p["rmean"][l].shape, init=p["rmean"][l])
            o["rvar", l + 1, s] = _Guarded(p["rvar"][l].shape, init=p["rvar"][l])
            for k, src in (("dw", "w"), ("dbias", "bias"), ("dgamma", "gamma"), ("dbeta", "beta")):
                o[k, l + 1, s] = _Guarded(p[src][l].shape)
            a.g[s].w[l], a.g[s].bias[l], a.g[s].gamma[l], a.g[s].beta[l] = (o[k, l + 1, s].ptr for k in ("dw", "dbias", "dgamma", "dbeta"))
    for g in range(G):
        s = R.param_set(c, g)
        a.img[g] = d_img[id(t["img"][g])].data_ptr()
        a.svec[g] = d_sv[id(t["svec"][g])].data_ptr() if S else None
        for l in range(L4):
            a.p[g].w[l], a.p[g].bias[l], a.p[g].gamma[l], a.p[g].beta[l] = (d_par[s][k][l].data_ptr() for k in ("w", "bias", "gamma", "beta"))
            if not c["null_running"]:
                a.p[g].running_mean[l], a.p[g].running_var[l] = o["rmean", l + 1, s].ptr, o["rvar", l + 1, s].ptr
        if c["want"][g]:
            o["dimg", g] = _Guarded((B, 3, 64, 64))
            a.dimg[g] = o["dimg", g].ptr
            if S:
                o["dsvec", g] = _Guarded((B, S))
                a.dsvec[g] = o["dsvec", g].ptr
    pl = R.plan(B, C, G)
    o["feat"], o["ws"], o["scr"] = _Guarded((G, B, C[L4], 4, 4)), _Guarded((pl["ws_total"],)), _Guarded((pl["scr_total"],))
    dfeat = _dev(t["dfeat"])
    keep.append(dfeat)
    a.feat, a.workspace, a.workspace_bytes = o["feat"].ptr, o["ws"].ptr, 4 * pl["ws_total"]
    a.dfeat, a.scratch, a.scratch_bytes = dfeat.data_ptr(), o["scr"].ptr, 4 * pl["scr_total"]
    return a, o, pl


def _run(L, c, t):
    """Forward and backward of a case on guarded buffers -> ({key: host array} as _trunkref.chain keys them, the raw buffers)."""
    from adaptiveisp_amd import _lib
    keep = []
    a, o, pl = _args(c, t, keep)
    G, B, C, S = c["G"], c["B"], c["C"], c["n_state"]
    ref = ctypes.byref(a)
    # the layout _trunkref.plan restates is the library's: the totals agree
    assert L.adaisp_trunk_train_workspace_bytes(ref) == 4 * pl["ws_per_g"] * G == 4 * pl["ws_total"], c["name"]
    assert L.adaisp_trunk_train_scratch_bytes(ref) == 4 * (pl["scr_per_g"] * G + pl["wpart_size"]), c["name"]
    with torch.cuda.device(DEV):
        _lib._check(L.adaisp_trunk_train_fwd(ref, _lib._stream()), "adaisp_trunk_train_fwd")
        _lib._check(L.adaisp_trunk_train_bwd(ref, _lib._stream()), "adaisp_trunk_train_bwd")
        torch.cuda.synchronize()
    name = c["name"]
    raw = {k: v.raw(f"{name} {k}").copy() for k, v in o.items()}
    got = {}
    for k, v in o.items():
        if k in ("ws", "scr", "feat"):
            continue
        if k[0] in ("rmean", "rvar") and c["null_running"]:
            s = k[2]
            assert np.array_equal(raw[k], t["params"][s][k[0]][k[1] - 1]), f"{name} {k}: written although the pointers are NULL"
            continue
        got[k] = v.read(f"{name} {k}")
    feat = o["feat"].read(f"{name} feat")
    ws = o["ws"].read(f"{name} workspace").reshape(G, pl["ws_per_g"])                   # every float of it is written
    scr = raw["scr"]
    for g in range(G):
        sc = scr[g * pl["scr_per_g"]:(g + 1) * pl["scr_per_g"]]
        for l in range(1, L4 + 1):
            H = 64 >> l
            n, shape = B * C[l] * H * H, (B, C[l], H, H)
            got["y", l, g] = ws[g, pl["y"][l]:pl["y"][l] + n].reshape(shape)
            got["a", l, g] = ws[g, pl["a"][l]:pl["a"][l] + n].reshape(shape) if l < L4 else feat[g]
            got["mean", l, g] = ws[g, pl["mean"][l]:pl["mean"][l] + C[l]]
            got["rstd", l, g] = ws[g, pl["rstd"][l]:pl["rstd"][l] + C[l]]
            got["dy", l, g] = sc[pl["dy"][l]:pl["dy"][l] + n].reshape(shape)
            if l < L4:
                got["da", l, g] = sc[pl["da"][l]:pl["da"][l] + n].reshape(shape)
        planes = sc[pl["da"][0]:]
        n = B * S * 4096 if c["want"][g] else 0                                         # channels 3.. of the first layer's gradient
        assert np.isnan(planes[n:]).all(), f"{name} instance {g}: the scratch past the state-plane gradients was written"
        if n:
            got["dplanes", g] = planes[:n].reshape(B, S, 64, 64)
        assert not np.isnan(sc[:pl["da"][0] + n]).any(), f"{name} instance {g}: part of dy / da not written"
    assert not np.isnan(scr[pl["wpart"]:]).any(), f"{name}: part of the weight-gradient partial region not written"
    return got, raw


_RUNS = {}


def _device_run(L, i):
    """Inputs and the device's buffers of case i, made once and shared by the tests of that case; a second run on fresh buffers
    is compared bit for bit at once (NaN filler included) and only the verdict kept."""
    if i not in _RUNS:
        c = R.CASES[i]
        t = R.inputs(c)
        got, raw = _run(L, c, t)
        raw2 = _run(L, c, t)[1]
        differ = [str(k) for k in raw if not np.array_equal(raw[k].view(np.int32), raw2[k].view(np.int32))]
        _RUNS[i] = (t, got, differ)
    return _RUNS[i]


IDS = [c["name"] for c in R.CASES]


def _emit(prefix):
    def emit(label, shares, what):
        shares = np.asarray(shares, dtype=np.float64)
        print(f"{what} {label}: largest share of the bound used {float(shares.max()):.4f}")
        close(f"{prefix}.{label}", shares, np.zeros_like(shares), rtol=0, atol=1.0, err_msg=what)
    return emit


@pytest.mark.parametrize("i", range(len(R.CASES)), ids=IDS)
def test_buffers_are_written_inside_their_guards_and_two_runs_give_equal_bits(L, i):
    t, got, differ = _device_run(L, i)                                                  # (the guards are asserted as it reads)
    assert not differ, f"{R.CASES[i]['name']}: {differ} differ between two runs"
    assert all(np.isfinite(v).all() for v in got.values())


@pytest.mark.parametrize("i", range(len(R.CASES)), ids=IDS)
def test_forward_stages_within_their_bounds(L, i):
    c = R.CASES[i]
    t, got, _ = _device_run(L, i)
    R.stage_shares(c, t, got, _emit("trunk_stages"), backward=False)
    if c["special"]:                                                                    # z exactly 0 takes the slope branch
        for g in range(c["G"]):
            assert c["special"] != True or abs(float(got["mean", 1, g][5])) > 900.0  # noqa: E712
            zero = np.ascontiguousarray(got["a", 2, g][:, 7]).view(np.uint32) & 0x7fffffff
            assert not zero.any(), "the all-zero channel's activation is not 0"


@pytest.mark.parametrize("i", range(len(R.CASES)), ids=IDS)
def test_backward_stages_within_their_bounds(L, i):
    c = R.CASES[i]
    t, got, _ = _device_run(L, i)

    R.stage_shares(c, t, got, _emit("trunk_stages"), forward=False)


@pytest.mark.parametrize("i", [k for k, c in enumerate(R.CASES) if c["B"] <= R.CHAIN_MAX_B],
                         ids=[c["name"] for c in R.CASES if c["B"] <= R.CHAIN_MAX_B])
def test_chain_against_float64_with_the_devices_masks(L, i):
    c = R.CASES[i]
    t, got, _ = _device_run(L, i)

    def emit(group, frac, what):
        frac = np.asarray(frac, dtype=np.float64)
        print(f"{what}: {float(frac.max()):.3e} of its scale (bound {R.CHAIN_FRAC[group]:.1e})")
        close(f"trunk_stages.chain.{group}", frac, np.zeros_like(frac), rtol=0, atol=R.CHAIN_FRAC[group], err_msg=what)
    R.chain_shares(c, t, got, emit)


# ---- what the entry points refuse ------------------------------------------------------------------------------------------------
_BASE = R._case("refusal-base", 2, 2, (16, 16, 16, 16), G=2, want=(0, 1))


def _set(field, value):
    return lambda a: setattr(a, field, value)


def _set_c(l, v):
    def f(a):
        a.C[l] = v
    return f


def _null_gamma(a):
    a.p[0].gamma[2] = None


def _null_grad(a):
    a.g[1].w[3] = None


def _dimg_alone(a):
    a.dsvec[1] = None


def _short(field):
    return lambda a: setattr(a, field, getattr(a, field) - 1)


# (what, change, return code, entry points that refuse it: a backward-only condition does not stop the forward)
REFUSED = [("C1=8", _set_c(1, 8), ESHAPE, "fb"), ("C2=24", _set_c(2, 24), ESHAPE, "fb"), ("C4=1040", _set_c(4, 1040), ESHAPE, "fb"),
           ("B=0", _set("B", 0), ESHAPE, "fb"), ("B=4097", _set("B", 4097), ESHAPE, "fb"), ("G=3", _set("G", 3), ESHAPE, "fb"),
           ("C0!=3+n_state", _set_c(0, 6), ESHAPE, "fb"), ("workspace-one-byte-short", _short("workspace_bytes"), ESHAPE, "fb"),
           ("scratch-one-byte-short", _short("scratch_bytes"), EINVAL, "b"),
           ("share_params-with-two-weight-sets", _set("share_params", 1), EINVAL, "fb"),
           ("dimg-without-dsvec", _dimg_alone, EINVAL, "b"), ("null-gamma", _null_gamma, EINVAL, "fb"),
           ("null-weight-gradient", _null_grad, EINVAL, "b")]


@pytest.mark.parametrize("what,change,rc,entries", REFUSED, ids=[r[0] for r in REFUSED])
def test_trunk_refuses_what_it_cannot_run(L, what, change, rc, entries):
    from adaptiveisp_amd import _lib
    keep = []
    a, o, _ = _args(_BASE, R.inputs(_BASE), keep)
    for v in o.values():                                                                # (the running statistics' initial values too)
        v.buf.fill_(float("nan"))
    change(a)
    with torch.cuda.device(DEV):
        rcs = tuple(fn(ctypes.byref(a), _lib._stream()) for e, fn in (("f", L.adaisp_trunk_train_fwd), ("b", L.adaisp_trunk_train_bwd))
                    if e in entries)
        torch.cuda.synchronize()
    assert rcs == (rc,) * len(entries), f"{what}: returned {rcs}"
    assert all(v.untouched() for v in o.values()), f"{what}: a refused call wrote to its buffers"
