"""Image gradients of the ISP kernels (adaisp_backward_image) against the reference's autograd, and the opt-in switch
`adaptiveisp_amd.image_grad()` through every Python entry point that applies a filter.

Fixture: tests/golden/filters_imggrad.npz (tests/golden/gen_imggrad.py, autograd of the reference itself). Caps (CAPS below):
pointwise and stencil ops 2e-6 of the gradient scale, NLM 5e-6 (121 offsets summed in another order); full size: GPU autograd of
oracle/torch_ref (NLM: the relu restatement of tests/test_imggrad_fixture.py, at one image: its autograd keeps 121 shifted
copies)."""
import numpy as np
import pytest
import torch

from _margins import close_scaled, vector_close
from test_imggrad_fixture import KEYS, NLM_TAGS, OPS, nlm_relu

pytestmark = pytest.mark.gpu


def dev():
    assert torch.cuda.is_available(), "run with -m gpu on the MI355X box"
    return torch.device("cuda:0")


def T(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev())


# Fractions of the gradient scale, tightened from the issue's 1e-5 (pointwise, stencils) and 1e-4 (NLM) to ~5x the largest
# error measured on the MI355X (4e-7 and 9e-7). Contrast: at a dark pixel (the fixture's x = 0.0005) -cos(pi L) * 0.5 + 0.5
# cancels to a few ulps, divided by L + 1e-6; the reference's own gradient there moves by ~3e-5 of the scale with the last
# ulp of its cos (ATen's cos is not the device's), so that op's cap is 5e-5.
CAPS = {"NLM": 5e-6, "Ct": 5e-5}


def cap(name):
    return CAPS.get(name, 2e-6)


def lib_grad(img, go, op, params, clip):
    from adaptiveisp_amd import _lib
    B = img.shape[0]
    ids = torch.full((B,), op, dtype=torch.int32, device=dev())
    g = _lib.backward_image(T(img), T(go), ids, T(params), clip=clip)
    torch.cuda.synchronize()
    return g.cpu().numpy()


@pytest.mark.parametrize("name", KEYS)
@pytest.mark.parametrize("mode", ["process", "forward"])
def test_matches_reference_autograd(golden, name, mode):
    g = golden("filters_imggrad")
    got = lib_grad(g["img"], g["grad_out"], OPS[name], g[f"{name}.param"], mode == "forward")
    close_scaled(f"image_grad:{name}", got, g[f"{name}.{mode}"], cap(name))


@pytest.mark.parametrize("tag", NLM_TAGS)
@pytest.mark.parametrize("mode", ["process", "forward"])
def test_nlm_wraparound(golden, tag, mode):
    g = golden("filters_imggrad")
    got = lib_grad(g[f"nlm.{tag}.img"], g[f"nlm.{tag}.grad_out"], OPS["NLM"], g[f"nlm.{tag}.h"], mode == "forward")
    close_scaled(f"image_grad:nlm_{tag}", got, g[f"nlm.{tag}.{mode}"], cap("NLM"))


def _packed(g, names):
    from adaptiveisp_amd import _lib
    p = np.zeros((len(names), _lib.MAX_PARAMS), np.float32)
    for i, n in enumerate(names):
        if n in OPS:
            row = g[f"{n}.param"][i % 2]
            p[i, :row.size] = row
    return p


def test_mixed_ids_equal_per_op_calls(golden):
    """One batch with every op, -1 and an id outside the enum: bit-identical to one call per image; zeros for the last two."""
    from adaptiveisp_amd import _lib
    g = golden("filters_imggrad")
    names = list(KEYS) + ["zero", "unknown"]
    ids = np.array([OPS[n] for n in KEYS] + [_lib.OP_ZERO, 99], np.int32)
    B = len(names)
    img = np.stack([g["img"][i % 2] for i in range(B)])
    go = np.stack([g["grad_out"][(i + 1) % 2] for i in range(B)])
    params = _packed(g, names)
    for clip in (False, True):
        mixed = _lib.backward_image(T(img), T(go), T(ids), T(params), clip=clip).cpu().numpy()
        for i in range(B):
            one = _lib.backward_image(T(img[i:i + 1]), T(go[i:i + 1]), T(ids[i:i + 1]), T(params[i:i + 1]), clip=clip)
            assert np.array_equal(mixed[i], one.cpu().numpy()[0]), names[i]
        assert not mixed[-2:].any()


# (relative L2, cosine). The sharpen pair's reference here is ATen's GPU convolution, whose sums round differently from the
# reference's CPU ones that the kernels follow bit for bit: at 22 M outputs a few land within an ulp of the clamp's ends and
# take the other side of the gate (one pixel moves the relative L2 by ~5e-4). USM's weights are not exact in either form.
FULL_BOUNDS = {"NLM": (2e-4, 0.9999999), "Shr": (3e-3, 0.999995), "ShrV2": (3e-3, 0.999995)}


def _full_size_inputs(B, seed):
    gen = torch.Generator(device="cpu").manual_seed(seed)
    x = torch.rand(B, 3, 720, 1280, generator=gen) ** 2.2 * 0.8
    x[:, :, :8] = torch.rand(B, 3, 8, 1280, generator=gen) * 1.4 - 0.2      # a band outside [0, 1]: every gate sees both sides
    go = torch.randn(B, 3, 720, 1280, generator=gen)
    return x.to(dev()), go.to(dev())


@pytest.mark.parametrize("name", KEYS)
def test_full_size_against_torch_autograd(golden, name):
    from adaptiveisp_amd import _lib
    from oracle import torch_ref
    g = golden("filters_imggrad")
    B = 1 if name == "NLM" else 8
    x, go = _full_size_inputs(B, 7 + OPS[name])
    p = T(np.concatenate([g[f"{name}.param"]] * 4)[:B])
    ids = torch.full((B,), OPS[name], dtype=torch.int32, device=dev())
    for clip in (False, True):
        got = _lib.backward_image(x, go, ids, p, clip=clip)
        xr = x.clone().requires_grad_(True)
        with torch.device(dev()):             # torch_ref builds its constant tensors without a device
            y = nlm_relu(xr, p) if name == "NLM" else torch_ref.process(OPS[name], xr, p)
            if clip:
                y = torch.clip(y, 0.0, 1.0)
            (y * go).sum().backward()
        vector_close(f"image_grad_full:{name}", got, xr.grad, *FULL_BOUNDS.get(name, (2e-5, 0.9999999)))
        del xr, y


def test_filter_forward_chain_under_switch(golden):
    """Tone -> Sharpen -> CCM as Filter.forward calls with learnable parameters: x.grad and the three parameter
    gradients of the reference's autograd (the fixture's chain)."""
    import adaptiveisp_amd
    from adaptiveisp_amd.config import cfg
    from adaptiveisp_amd.isp import filters as F
    g = golden("filters_imggrad")
    x = T(g["img"]).requires_grad_(True)
    ps = {k: T(g[f"{k}.param"]).requires_grad_(True) for k in ("T", "Shr", "CCM")}
    with adaptiveisp_amd.image_grad():
        y = x
        for k, cls in (("T", F.ToneFilter), ("Shr", F.SharpenFilter), ("CCM", F.CCMFilter)):
            y = cls(cfg).forward(y, specified_parameter=ps[k])[0]
    (y * T(g["grad_out"])).sum().backward()            # outside the block: the state was taken at forward time
    close_scaled("image_grad:chain_x", x.grad, g["chain.x"], cap("chain"))
    for k in ("T", "Shr", "CCM"):
        close_scaled(f"image_grad:chain_{k}", ps[k].grad, g[f"chain.{k}"], 2e-4)


def test_switch_is_opt_in_and_read_at_forward_time(golden):
    import adaptiveisp_amd
    from adaptiveisp_amd.config import cfg
    from adaptiveisp_amd.isp import filters as F
    g = golden("filters_imggrad")
    G = T(g["grad_out"])
    p = T(g["E.param"]).requires_grad_(True)
    x = T(g["img"]).requires_grad_(True)
    y = F.ExposureFilter(cfg).forward(x, specified_parameter=p)[0]
    with adaptiveisp_amd.image_grad():                  # on at backward time only: the forward decided
        with pytest.raises(NotImplementedError, match="image_grad"):
            (y * G).sum().backward()
    with adaptiveisp_amd.image_grad():
        y = F.ExposureFilter(cfg).forward(x, specified_parameter=p)[0]
        with adaptiveisp_amd.image_grad(enabled=False):
            z = F.ExposureFilter(cfg).forward(x, specified_parameter=p)[0]
    assert not adaptiveisp_amd.isp.image_grad_enabled()
    (y * G).sum().backward()
    close_scaled("image_grad:switch", x.grad, g["E.forward"], cap("E"))
    with pytest.raises(NotImplementedError):
        (z * G).sum().backward()


def test_entry_points_under_switch(golden):
    """Filter.process, the sharpen wrappers, NonLocalMeansGray(11, 5) and the Agent path (device op ids)."""
    import adaptiveisp_amd
    from adaptiveisp_amd import _lib
    from adaptiveisp_amd.config import cfg
    from adaptiveisp_amd.isp import filters as F, sharpen
    from adaptiveisp_amd.isp.denoise import NonLocalMeansGray
    from adaptiveisp_amd.isp.isp_function import isp_apply_selected
    g = golden("filters_imggrad")
    G = T(g["grad_out"])

    def grad_of(fn):
        x = T(g["img"]).requires_grad_(True)
        with adaptiveisp_amd.image_grad():
            y = fn(x)
        (y * G).sum().backward()
        return x.grad

    p = lambda k: T(g[f"{k}.param"])          # noqa: E731
    close_scaled("image_grad:entry_process", grad_of(lambda x: F.GammaFilter(cfg).process(x, p("G"))), g["G.process"], cap("G"))
    close_scaled("image_grad:entry_sharpen", grad_of(lambda x: sharpen.adjust_sharpness(x, p("Shr"))), g["Shr.process"], cap("Shr"))
    close_scaled("image_grad:entry_sharpen", grad_of(lambda x: sharpen.sharpness(x, p("ShrV2"))), g["ShrV2.process"], cap("ShrV2"))
    us = p("USM")
    close_scaled("image_grad:entry_sharpen", grad_of(lambda x: sharpen.unsharp_mask(x, us[:, 0], us[:, 1])), g["USM.process"],
                 cap("USM"))
    close_scaled("image_grad:entry_nlm", grad_of(lambda x: NonLocalMeansGray(11, 5)(x.clamp(0, 1), p("NLM"))),
                 g["NLM.process"], cap("NLM"))
    names = ["C", "Sp"]
    ids = T(np.array([OPS[n] for n in names], np.int32))
    packed = T(_packed(g, names))
    got = grad_of(lambda x: isp_apply_selected(x, packed, ids, clip=True))
    ref = np.stack([g["C.forward"][0], g["Sp.forward"][1]])
    close_scaled("image_grad:entry_selected", got, ref, cap("Sp"))
    # other NLM window sizes keep raising (out of scope)
    x = T(g["img"]).clamp(0, 1).requires_grad_(True)
    with adaptiveisp_amd.image_grad(), pytest.raises(NotImplementedError):
        NonLocalMeansGray(7, 3)(x, p("NLM"))
    assert _lib.ABI_VERSION == 9


def test_graph_capture_replays_eager(golden):
    """Forward + image backward captured on one stream (no allocation, no host sync inside the calls) replay to the
    eager result."""
    from adaptiveisp_amd import _lib
    g = golden("filters_imggrad")
    names = list(KEYS) + ["zero"]
    B = len(names)
    img = T(np.stack([g["img"][i % 2] for i in range(B)]))
    go = T(np.stack([g["grad_out"][i % 2] for i in range(B)]))
    ids = T(np.array([OPS[n] for n in KEYS] + [_lib.OP_ZERO], np.int32))
    params = T(_packed(g, names))

    def step():
        out = _lib.forward(img, ids, params, clip=True)
        return out, _lib.backward_image(out, go, ids, params, clip=True)

    eager_out, eager_grad = step()
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        step()
    torch.cuda.current_stream().wait_stream(s)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        cap_out, cap_grad = step()
    cap_grad.zero_()
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(cap_out, eager_out)
    assert torch.equal(cap_grad, eager_grad)


def test_argument_checks(golden):
    import ctypes
    from adaptiveisp_amd import _lib
    L = _lib.load()
    g = golden("filters_imggrad")
    img, go = T(g["img"]), T(g["grad_out"])
    ids = torch.zeros(2, dtype=torch.int32, device=dev())
    p = T(g["E.param"])
    B, _, H, W = img.shape
    n = int(L.adaisp_backward_image_workspace_bytes(B, H, W))
    assert n >= 16 * B * H * W
    ws = torch.empty(n // 4, device=dev())
    s = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    args = lambda out, nbytes: (img.data_ptr(), go.data_ptr(), ids.data_ptr(), p.data_ptr(), 1, out, ws.data_ptr(),  # noqa
                                nbytes, B, H, W, 1, s)
    assert L.adaisp_backward_image(*args(img.data_ptr(), n)) == -3        # grad_img aliases img
    assert L.adaisp_backward_image(*args(go.data_ptr(), n)) == -3         # ... or grad_out
    out = torch.empty_like(img)
    assert L.adaisp_backward_image(*args(out.data_ptr(), n - 4)) == -1    # workspace too small
    assert L.adaisp_backward_image(*args(None, n)) == -1
    assert L.adaisp_backward_image(*args(out.data_ptr(), n)) == 0
