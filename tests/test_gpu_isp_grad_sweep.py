"""Parameter and image gradients of the ISP kernels (adaisp_backward_params, adaisp_backward_image) against float64 at the
shapes where the kernels go wrong: ragged tiles, tile seams, reflect folds, NLM wrap-around, several workgroups per image
and the grid-stride loops. References: tests/_gradref.py (oracle/torch_ref in float64 on ATen; pinned to the reference
project's autograd by tests/test_gradref_fixture.py). Outputs whose kink is decided by arithmetic get grad_out = 0 in
what both sides receive (_gradref.ambiguity_masks); the masked share is asserted below 0.1% per case.

Parameter gradients: |got - ref_k| <= PARAM_CAP * S_k, S_k = sum |grad_out * d out / d p_k| (the mass an fp32 sum's error
scales with). Image gradients: |got - ref| <= cap * max(1, max |ref|), element-wise (test_gpu_image_grad.py's caps)."""
import ctypes
import time

import numpy as np
import pytest
import torch

import _gradref
from _margins import NOTES, close, close_scaled
from oracle.torch_ref import NUM_PARAMS
from test_gpu_parity import rand_params
from test_imggrad_fixture import KEYS, OPS

pytestmark = pytest.mark.gpu

SHAPES = [
    (1, 3, 3),          # smallest accepted size: every tap is on the frame or folds; smaller than NLM's 11 x 11 window
    (2, 4, 5),          # USM's fold rows 1-2 and H-3..H-2 touch
    (1, 5, 6),          # ... and overlap
    (1, 9, 10),         # NLM's roll wraps more than once
    (3, 17, 65),        # one row past a 16-row tile, one column past 64; odd plane: the scalar pointwise path
    (1, 33, 61),        # one past the NLM parameter kernel's 32 x 60 tile
    (2, 47, 127),       # ragged last tile in every family (16, 24, 32 rows; 32, 60, 64 columns)
    (1, 130, 250),      # several ragged tiles each way; about 16 parameter workgroups per image
    (8, 512, 512),      # config 4's per-rank training shape
    (2, 720, 1280),     # the benchmark shape, element-wise
    (1, 1080, 1920),    # above 2^20 px: the parameter kernels reach their 512 workgroups and the image pointwise
    (1, 2160, 3840),    # kernel its 1024, so both grid-stride loops run
]
NLM_IMAGE_MAX = (1, 130, 250)    # reverse-mode float64 through 121 rolls keeps every shifted copy
MODES = ("process", "forward")
MAX_MASKED = 1e-3

# Fraction of the summation mass S_k (module docstring).
PARAM_CAP = 1e-5
# Image gradients: test_gpu_image_grad.py's caps (Contrast: the dark-pixel cancellation described there).
IMG_CAPS = {"NLM": 5e-6, "Ct": 5e-5}


def dev():
    assert torch.cuda.is_available(), "run with -m gpu on the MI355X box"
    return torch.device("cuda:0")


def sweep_inputs(B, H, W, seed):
    """x in [0.04, 0.96] (no output near a clip by construction), plus one pixel in 4099 set to an exact-input case
    the header gives a convention for: a tone / colour breakpoint, Gamma's 0.001, above 1, below 0, a channel tie,
    0 and 1. grad_out ~ N(0, 1)."""
    gen = torch.Generator().manual_seed(seed)
    x = torch.rand(B, 3, H, W, generator=gen) * 0.92 + 0.04
    go = torch.randn(B, 3, H, W, generator=gen)
    plane = H * W
    flat = x.view(B, 3, plane)
    for j, q in enumerate(range(1000, B * plane, 4099)):
        b, r, c = q // plane, q % plane, (j // 7) % 3
        kind = j % 7
        if kind == 4:
            flat[b, (c + 1) % 3, r] = flat[b, c, r]
        else:
            flat[b, c, r] = (((j // 21) % 7 + 1) / 8, 0.001, 1.25, -0.2, None, 0.0, 1.0)[kind]
    return x.to(dev()), go.to(dev())


_INPUTS = {}


def inputs(shape):
    if shape not in _INPUTS:
        _INPUTS.clear()
        torch.cuda.empty_cache()
        _INPUTS[shape] = sweep_inputs(*shape, seed=sum(shape))
    return _INPUTS[shape]


def params_for(op, B, seed):
    return torch.from_numpy(rand_params(op, B, np.random.default_rng(seed)).astype(np.float32)).to(dev())


def masked_grad_out(op, x, p, go, mode, what):
    m = _gradref.ambiguity_masks(op, x, p)[mode]
    share = float(m.double().mean())
    assert share < MAX_MASKED, f"{what}: {share:.2e} of the outputs masked"
    return go.masked_fill(m, 0.0), share


def check_params(label, got, ref, mass, what):
    """|got - ref| <= PARAM_CAP * S, recorded on the S-normalised tensors (as close_scaled does)."""
    got = got.double()
    zero = mass == 0                              # every term is exactly 0: the gates and the structure decide
    assert torch.equal(got[zero], torch.zeros_like(got[zero])), f"{what}: nonzero where every term is 0"
    s = torch.where(zero, torch.ones_like(mass), mass)
    close(label, got / s, ref / s, rtol=0.0, atol=PARAM_CAP, err_msg=what)


def _id(case):
    (B, H, W), name = case
    return f"{B}x{H}x{W}-{name}"


PARAM_CASES = [(s, n) for s in SHAPES for n in KEYS]
IMAGE_CASES = [(s, n) for s in SHAPES for n in KEYS if n != "NLM" or s[1] * s[2] <= NLM_IMAGE_MAX[1] * NLM_IMAGE_MAX[2]]
MASKED = {}


@pytest.fixture(scope="module", autouse=True)
def _budget():
    torch.cuda.reset_peak_memory_stats()
    t0 = time.perf_counter()
    yield
    NOTES.append(f"grad sweep: {time.perf_counter() - t0:.1f} s, peak device memory "
                 f"{torch.cuda.max_memory_allocated() / 2**30:.2f} GiB, largest masked share "
                 f"{max(MASKED.values(), default=0.0):.2e} ({max(MASKED, key=MASKED.get, default='-')})")
    _INPUTS.clear()


@pytest.mark.parametrize("case", PARAM_CASES, ids=_id)
def test_param_grads(case):
    from adaptiveisp_amd import _lib
    shape, name = case
    op, B = OPS[name], shape[0]
    x, go = inputs(shape)
    p = params_for(op, B, 11 + op)
    ids = torch.full((B,), op, dtype=torch.int32, device=dev())
    for mode in MODES:
        what = f"{name} {mode} {shape}"
        G, MASKED[what] = masked_grad_out(op, x, p, go, mode, what)
        got = _lib.backward_params(x, G, ids, p, clip=mode == "forward")
        ref, mass = _gradref.param_grads(op, x, p, G, mode == "forward")
        check_params(f"grad_sweep_params:{name}", got[:, :NUM_PARAMS[op]], ref, mass, what)


@pytest.mark.parametrize("case", IMAGE_CASES, ids=_id)
def test_image_grads(case):
    from adaptiveisp_amd import _lib
    shape, name = case
    op, B = OPS[name], shape[0]
    x, go = inputs(shape)
    p = params_for(op, B, 11 + op)
    ids = torch.full((B,), op, dtype=torch.int32, device=dev())
    for mode in MODES:
        what = f"{name} {mode} {shape}"
        G, _ = masked_grad_out(op, x, p, go, mode, what)
        got = _lib.backward_image(x, G, ids, p, clip=mode == "forward")
        ref = _gradref.image_grad(op, x, p, G, mode == "forward")
        close_scaled(f"grad_sweep_image:{name}", got, ref, IMG_CAPS.get(name, 2e-6), err_msg=what)
        del got, ref


# ---- mixed ids at the training shape --------------------------------------------------------------------------------
TRAIN = (8, 512, 512)
MIXED = ((OPS["E"], OPS["G"], OPS["CCM"], OPS["Shr"], OPS["NLM"], OPS["T"], OPS["Ct"], OPS["Sp"]),
         (OPS["BW"], OPS["W"], OPS["USM"], OPS["ShrV2"], OPS["C"], -1, 99, OPS["USM"]))
NAMES = {v: k for k, v in OPS.items()}


def packed_params(ops, stride, seed):
    """[B, stride]: row b = the parameters of ops[b], then junk (3.0) in the columns past its count; ids -1 and 99: junk."""
    rng = np.random.default_rng(seed)
    p = np.full((len(ops), stride), 3.0, np.float32)
    for b, op in enumerate(ops):
        if op in NUM_PARAMS:
            p[b, :NUM_PARAMS[op]] = rand_params(op, 1, rng)[0]
    return torch.from_numpy(p).to(dev())


def row_checks(label, x, go, ops, packed, mode, got_p, got_i):
    """Each row against its own op's float64 reference; exact zeros past an op's count and for ids outside the enum."""
    clip = mode == "forward"
    for b, op in enumerate(ops):
        if op not in NUM_PARAMS:
            assert not got_p[b].any() and not got_i[b].any(), f"{label}: id {op} row {b} is not zero"
            continue
        n, name, what = NUM_PARAMS[op], NAMES[op], f"{label} {NAMES[op]} row {b} {mode}"
        assert not got_p[b, n:].any(), f"{what}: columns past {n} are not zero"
        xb, gb, pb = x[b:b + 1], go[b:b + 1], packed[b:b + 1]
        ref, mass = _gradref.param_grads(op, xb, pb, gb, clip)
        check_params(f"grad_sweep_params:{name}", got_p[b:b + 1, :n], ref, mass, what)
        ref_i = _gradref.image_grad(op, xb, pb, gb, clip)
        close_scaled(f"grad_sweep_image:{name}", got_i[b:b + 1], ref_i, IMG_CAPS.get(name, 2e-6), err_msg=what)
        del ref_i


def mask_rows(x, go, ops, packed, mode):
    rows = []
    for b, op in enumerate(ops):
        if op in NUM_PARAMS:
            g, _ = masked_grad_out(op, x[b:b + 1], packed[b:b + 1], go[b:b + 1], mode, f"mixed {NAMES[op]} row {b}")
            rows.append(g)
        else:
            rows.append(go[b:b + 1])
    return torch.cat(rows)


@pytest.mark.parametrize("call", (0, 1))
@pytest.mark.parametrize("stride", ("packed", 32))
def test_mixed_ids_training_shape(call, stride):
    """One call per id set at 8 x 512 x 512; stride = the Agent's packed width (the widest op of the set) or 32."""
    from adaptiveisp_amd import _lib
    ops = MIXED[call]
    width = max(NUM_PARAMS[o] for o in ops if o in NUM_PARAMS) if stride == "packed" else stride
    x, go = inputs(TRAIN)
    packed = packed_params(ops, width, 40 + call)
    ids = torch.tensor(ops, dtype=torch.int32, device=dev())
    for mode in MODES:
        G = mask_rows(x, go, ops, packed, mode)
        got_p = _lib.backward_params(x, G, ids, packed, clip=mode == "forward")
        got_i = _lib.backward_image(x, G, ids, packed, clip=mode == "forward")
        torch.cuda.synchronize()
        row_checks(f"mixed call {call} stride {width}", x, G, ops, packed, mode, got_p, got_i)


# ---- the C-ABI's promises, called through ctypes --------------------------------------------------------------------
SENTINEL = -12345.0
ALL_IDS = tuple(range(13)) + (-1, 99)


def _fenced(n, pad, fill):
    """A buffer of pad + n + pad floats: sentinels around n floats of `fill`. Returns (buffer, the inner view)."""
    buf = torch.full((pad + n + pad,), SENTINEL, device=dev())
    buf[pad:pad + n] = fill
    return buf, buf[pad:pad + n]


def _fence_intact(buf, n, pad):
    s = torch.full((pad,), SENTINEL, device=dev())
    return torch.equal(buf[:pad], s) and torch.equal(buf[pad + n:], s)


@pytest.mark.parametrize("mode", MODES)
def test_outputs_are_written_in_place_and_only_there(mode):
    """grad_params pre-filled with NaN gives the fresh call's result ("zero-filled by the callee"); grad_img pre-filled
    with NaN is written in full; sentinels around both are untouched."""
    from adaptiveisp_amd import _lib
    L = _lib.load()
    B, H, W = len(ALL_IDS), 17, 65
    x, go = sweep_inputs(B, H, W, seed=5)
    stride = 32
    packed = packed_params(ALL_IDS, stride, 7)
    ids = torch.tensor(ALL_IDS, dtype=torch.int32, device=dev())
    flags = _lib.CLIP01 if mode == "forward" else 0
    s = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    fresh_p = _lib.backward_params(x, go, ids, packed, clip=mode == "forward")
    fresh_i = _lib.backward_image(x, go, ids, packed, clip=mode == "forward")

    pad, n_p, n_i = 4096, B * stride, x.numel()
    buf_p, gp = _fenced(n_p, pad, float("nan"))
    L.adaisp_backward_params(x.data_ptr(), go.data_ptr(), ids.data_ptr(), packed.data_ptr(), stride, gp.data_ptr(),
                             B, H, W, flags, s)
    nbytes = int(L.adaisp_backward_image_workspace_bytes(B, H, W))
    ws = torch.empty(nbytes // 4, device=dev())
    buf_i, gi = _fenced(n_i, pad, float("nan"))
    assert L.adaisp_backward_image(x.data_ptr(), go.data_ptr(), ids.data_ptr(), packed.data_ptr(), stride, gi.data_ptr(),
                                   ws.data_ptr(), nbytes, B, H, W, flags, s) == 0
    torch.cuda.synchronize()
    assert torch.equal(gp.view(B, stride), fresh_p)
    assert torch.equal(gi.view(B, 3, H, W), fresh_i)
    assert _fence_intact(buf_p, n_p, pad) and _fence_intact(buf_i, n_i, pad)


@pytest.mark.parametrize("mode", MODES)
def test_unaligned_pointers_take_the_scalar_path(mode):
    """img, grad_out and grad_img one float past 16-byte alignment, at a plane that is a multiple of 4: the pointwise
    image gradient runs its scalar path; every row against its float64 reference."""
    from adaptiveisp_amd import _lib
    L = _lib.load()
    ops = ALL_IDS
    B, H, W = len(ops), 20, 64
    x, go = sweep_inputs(B, H, W, seed=9)
    stride = 24
    packed = packed_params(ops, stride, 13)
    ids = torch.tensor(ops, dtype=torch.int32, device=dev())
    G = mask_rows(x, go, ops, packed, mode)
    n = x.numel()
    bx, by, bo = (torch.full((n + 1 + 4,), SENTINEL, device=dev()) for _ in range(3))
    bx[1:1 + n], by[1:1 + n] = x.flatten(), G.flatten()
    xo, go_o, out = bx[1:1 + n], by[1:1 + n], bo[1:1 + n]
    assert xo.data_ptr() % 16 == 4 and out.data_ptr() % 16 == 4
    nbytes = int(L.adaisp_backward_image_workspace_bytes(B, H, W))
    ws = torch.empty(nbytes // 4, device=dev())
    s = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    assert L.adaisp_backward_image(xo.data_ptr(), go_o.data_ptr(), ids.data_ptr(), packed.data_ptr(), stride,
                                   out.data_ptr(), ws.data_ptr(), nbytes, B, H, W,
                                   _lib.CLIP01 if mode == "forward" else 0, s) == 0
    torch.cuda.synchronize()
    assert bo[0].item() == SENTINEL and torch.equal(bo[1 + n:], torch.full((4,), SENTINEL, device=dev()))
    got_i = out.view(B, 3, H, W)
    got_p = _lib.backward_params(x, G, ids, packed, clip=mode == "forward")
    row_checks("unaligned", x, G, ops, packed, mode, got_p, got_i)
