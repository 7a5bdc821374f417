"""tests/_gradref.py (the float64 gradient reference of tests/test_gpu_isp_grad_sweep.py) pinned to the reference project's
own numbers: its fp32 autograd in filters_grad.npz (parameter gradients) and filters_imggrad.npz (image gradients). Plus
the ambiguity mask: it takes the arithmetic kinks and leaves the exact-input conventions alone."""
import numpy as np
import pytest
import torch

import _gradref
from oracle import torch_ref
from test_imggrad_fixture import KEYS, NLM_TAGS, OPS, assert_scaled


def _t(a):
    return torch.from_numpy(np.ascontiguousarray(a)).double()


@pytest.mark.parametrize("name", KEYS)
@pytest.mark.parametrize("mode", ["process", "forward"])
def test_param_grads_reproduce_fixture(golden, name, mode):
    g, gg = golden("filters"), golden("filters_grad")
    ref, mass = _gradref.param_grads(OPS[name], _t(g["img"]), _t(g[f"{name}.param"]), _t(gg["grad_out"]), mode == "forward")
    want = gg[f"{name}.{mode}"]
    assert ref.shape == want.shape
    err = np.abs(ref.numpy() - want)
    assert (err <= 1e-6 * mass.numpy()).all(), f"worst {float((err / mass.numpy()).max()):.3g} of S"


# The fixture is fp32 autograd: at the outputs the ambiguity mask names, it may take the other side of a kink (the
# maximum ties of Sp in row 0, Color's forward clip at 1). Elements those outputs reach (the same pixel, or 2 px for the
# stencils) are left out, and nothing else may differ: that also checks that the mask names every such output.
# test_imggrad_fixture.py's 1e-6 of the scale, except Contrast: at the fixture's dark pixel (x = 0.0005) the fixture's own
# fp32 gradient is 1.5e-5 of the scale away from float64 (the cancellation in -cos(pi L) * 0.5 + 0.5 that
# test_gpu_image_grad.py's CAPS describes), so it keeps that file's 5e-5.
IMG_CAPS = {"Ct": 5e-5}


@pytest.mark.parametrize("name", KEYS)
@pytest.mark.parametrize("mode", ["process", "forward"])
def test_image_grads_reproduce_fixture(golden, name, mode):
    g = golden("filters_imggrad")
    x, p = _t(g["img"]), _t(g[f"{name}.param"])
    got = _gradref.image_grad(OPS[name], x, p, _t(g["grad_out"]), mode == "forward")
    masked = _gradref.ambiguity_masks(OPS[name], x, p)[mode].any(dim=1, keepdim=True).double()
    if name == "NLM":
        assert not masked.any()
    if name in ("Shr", "ShrV2", "USM"):
        masked = torch.nn.functional.max_pool2d(masked, 5, stride=1, padding=2)
    reach = masked.bool().expand_as(x)
    assert reach.double().mean() < 0.1        # the fixture's image puts many pixels on 0, 1 and the breakpoints on purpose
    keep = ~reach.numpy()
    assert_scaled(got.numpy() * keep, g[f"{name}.{mode}"] * keep, IMG_CAPS.get(name, 1e-6))


@pytest.mark.parametrize("tag", NLM_TAGS)
@pytest.mark.parametrize("mode", ["process", "forward"])
def test_nlm_image_grads_reproduce_fixture(golden, tag, mode):
    g = golden("filters_imggrad")
    got = _gradref.image_grad(OPS["NLM"], _t(g[f"nlm.{tag}.img"]), _t(g[f"nlm.{tag}.h"]), _t(g[f"nlm.{tag}.grad_out"]),
                              mode == "forward")
    assert_scaled(got.numpy(), g[f"nlm.{tag}.{mode}"], 1e-6)


def test_default_dtype_is_restored():
    prev = torch.get_default_dtype()
    with pytest.raises(RuntimeError):
        with _gradref.float64("cpu"):
            assert torch.get_default_dtype() == torch.float64
            raise RuntimeError
    assert torch.get_default_dtype() == prev


def _img(*rgb):
    """[1,3,1,len] image from per-channel rows."""
    return torch.tensor([[[list(c)] for c in rgb]], dtype=torch.float64)


def test_mask_takes_arithmetic_kinks():
    p1 = torch.tensor([[0.5]], dtype=torch.float64)
    # Contrast: luminance 1 - 1e-5 (masked) and 0.5 (not)
    x = _img([1.0, 0.5], [1.0 - 1e-5 / 0.67, 0.5], [1.0, 0.5])
    m = _gradref.ambiguity_masks(torch_ref.CT, x, p1)
    assert m["process"][0, :, 0, 0].all() and not m["process"][0, :, 0, 1].any()
    # SaturationPlus: hue 1/6 + 1e-6 (sector 0 / 1 is arithmetic) and 1/12
    d = 0.5
    x = _img([0.75, 0.75], [0.25 + d * (1 + 6e-6), 0.25 + d / 2], [0.25, 0.25])
    m = _gradref.ambiguity_masks(torch_ref.SP, x, p1)
    assert m["process"][0, :, 0, 0].all() and not m["process"][0, :, 0, 1].any()
    # Exposure: the output clip decides only in forward mode
    x = _img([0.5 - 1e-6, 0.25], [0.25, 0.25], [0.25, 0.25])
    m = _gradref.ambiguity_masks(torch_ref.E, x, torch.tensor([[1.0]], dtype=torch.float64))
    assert not m["process"].any() and m["forward"][0, 0, 0, 0] and int(m["forward"].sum()) == 1
    # Sharpen: the value before the clamp is 1 + 1e-6 at the centre of a 3 x 3 image
    x = torch.full((1, 3, 3, 3), 0.5, dtype=torch.float64)
    x[0, :, 1, 1] = 0.5 + (0.5 + 1e-6) / 2.0
    m = _gradref.ambiguity_masks(torch_ref.SHRV2, x, torch.tensor([[1.0]], dtype=torch.float64))
    # centre: 0.5 + e + (e - 5e/13) with e = 0.25 + 5e-7 is not 1: check the mask against the value itself
    with _gradref.float64("cpu"):
        v = x + (x - torch_ref._blur3(x))
    assert torch.equal(m["process"], ((v - 1).abs() < _gradref.AMBIGUOUS) | (v.abs() < _gradref.AMBIGUOUS))
    assert torch.equal(m["forward"], m["process"])


def test_mask_leaves_exact_conventions():
    """Tone breakpoints, Gamma's 0.001 clip, input clips and channel ties are exact: never masked."""
    x = _img([k / 8 for k in range(1, 8)] + [0.001, -0.2, 1.3, 0.1, 0.2],
             [0.3] * 7 + [0.3, 0.3, 0.3, 0.1, 0.2],
             [0.2] * 7 + [0.2, 0.2, 0.2, 0.4, 0.2])
    for op, p in ((torch_ref.T, torch.full((1, 8), 1.0, dtype=torch.float64)),
                  (torch_ref.G, torch.tensor([[1.7]], dtype=torch.float64))):
        m = _gradref.ambiguity_masks(op, x, p)
        assert not m["process"].any()
    m = _gradref.ambiguity_masks(torch_ref.SP, x, torch.tensor([[0.5]], dtype=torch.float64))
    assert not m["process"][0, :, 0, -2:].any()          # the tie r == g < b and a grey pixel: sector from exact values
