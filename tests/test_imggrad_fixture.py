"""The image-gradient fixture (tests/golden/filters_imggrad.npz, autograd of the reference itself) against autograd of the
torch-CPU restatement: pins the fixture and the subgradient conventions the HIP image backward is held to.

oracle/torch_ref.nlm clamps the patch distance with clamp(min=0) where the reference uses relu; at D == 0 (the zero
offset, flat patches) their backward differs (inf * 1 against relu's 0), so the NLM entries are checked against the
relu form below. tests/test_gpu_image_grad.py uses the same restatement at full size."""
import math

import numpy as np
import pytest
import torch

from oracle import torch_ref

KEYS = ("E", "G", "CCM", "Shr", "NLM", "T", "Ct", "Sp", "BW", "W", "USM", "ShrV2", "C")
OPS = {k: i for i, k in enumerate(KEYS)}          # include/adaisp.h op codes, filters.npz keys
NLM_TAGS = ("a", "odd", "const")


def nlm_relu(img, h, search=11, patch=5):
    """DenoiseFilter.process (clip, then NonLocalMeansGray(11, 5)) with the reference's relu before the sqrt
    (isp/denoise.py:113); whole-tensor rolls like torch_ref.nlm."""
    hh = torch.relu(h.reshape(-1, 1, 1, 1)) + 1e-8
    x = torch.clip(img, 0.0, 1.0)
    y = 0.299 * x[:, 0:1] + 0.587 * x[:, 1:2] + 0.114 * x[:, 2:3]
    r, pr = search // 2, patch // 2
    num, den = torch.zeros_like(x), torch.zeros_like(y)
    for dx in range(-r, r + 1):
        for dy in range(-r, r + 1):
            xs = torch.roll(x, shifts=(dy, dx), dims=(2, 3))
            sq = (y - torch.roll(y, shifts=(dy, dx), dims=(2, 3))) ** 2
            dist = torch.zeros_like(sq)
            for bx in range(-pr, pr + 1):
                for by in range(-pr, pr + 1):
                    dist = dist + torch.roll(sq, shifts=(by, bx), dims=(2, 3))
            w = torch.exp(-torch.sqrt(torch.relu(dist)) / hh)
            num = num + xs * w
            den = den + w
    return torch.clamp(num / den, 0.0, 1.0)


def image_grad(fn, img, grad_out, clip):
    x = torch.as_tensor(img).clone().requires_grad_(True)
    y = fn(x)
    if clip:
        y = torch.clip(y, 0.0, 1.0)
    (y * torch.as_tensor(grad_out)).sum().backward()
    return x.grad.numpy()


def assert_scaled(got, ref, frac):
    scale = max(1.0, float(np.abs(ref).max()))
    assert np.isfinite(got).all()
    err = float(np.abs(got - ref).max())
    assert err <= frac * scale, f"max |diff| {err:.3g} > {frac:g} x scale {scale:.3g}"


def test_fixture_has_every_key(golden):
    g = golden("filters_imggrad")
    want = {"img", "grad_out", "chain.x", "chain.T", "chain.Shr", "chain.CCM"}
    want |= {f"{k}.{s}" for k in KEYS for s in ("param", "process", "forward")}
    want |= {f"nlm.{t}.{s}" for t in NLM_TAGS for s in ("img", "h", "grad_out", "process", "forward")}
    assert want <= set(g.files), sorted(want - set(g.files))
    for k in g.files:
        assert np.isfinite(g[k]).all(), k
    assert np.array_equal(g["img"], golden("filters")["img"])
    assert np.array_equal(g["grad_out"], golden("filters_grad")["grad_out"])


@pytest.mark.parametrize("name", [k for k in KEYS if k != "NLM"])
@pytest.mark.parametrize("mode", ["process", "forward"])
def test_torch_ref_autograd_reproduces_fixture(golden, name, mode):
    g = golden("filters_imggrad")
    p = torch.from_numpy(g[f"{name}.param"])
    got = image_grad(lambda x: torch_ref.process(OPS[name], x, p), g["img"], g["grad_out"], mode == "forward")
    assert_scaled(got, g[f"{name}.{mode}"], 1e-6)


@pytest.mark.parametrize("mode", ["process", "forward"])
def test_relu_nlm_reproduces_fixture(golden, mode):
    g = golden("filters_imggrad")
    cases = [(g["img"], g["NLM.param"], g["grad_out"], g[f"NLM.{mode}"])]
    cases += [(g[f"nlm.{t}.img"], g[f"nlm.{t}.h"], g[f"nlm.{t}.grad_out"], g[f"nlm.{t}.{mode}"]) for t in NLM_TAGS]
    for img, h, go, ref in cases:
        got = image_grad(lambda x: nlm_relu(x, torch.from_numpy(h)), img, go, mode == "forward")
        assert_scaled(got, ref, 1e-6)


def test_const_patch_has_zero_distances(golden):
    """The `const` case really reaches D == 0 away from the zero offset (where clamp(min=0) and relu differ)."""
    g = golden("filters_imggrad")
    x = torch.clip(torch.from_numpy(g["nlm.const.img"]), 0, 1)
    y = 0.299 * x[:, 0:1] + 0.587 * x[:, 1:2] + 0.114 * x[:, 2:3]
    d = sum(torch.roll((y - torch.roll(y, (0, 2), (2, 3))) ** 2, (by, bx), (2, 3)) for bx in range(-2, 3) for by in range(-2, 3))
    assert int((d == 0).sum()) > 0
    # the torch_ref form is NaN there: the fixture needs the relu restatement
    bad = image_grad(lambda t: torch_ref.nlm(t, torch.from_numpy(g["nlm.const.h"])), g["nlm.const.img"],
                     g["nlm.const.grad_out"], False)
    assert not np.isfinite(bad).all()


def test_chain_matches_fixture(golden):
    g = golden("filters_imggrad")
    x = torch.from_numpy(g["img"]).clone().requires_grad_(True)
    ps = {k: torch.from_numpy(g[f"{k}.param"]).clone().requires_grad_(True) for k in ("T", "Shr", "CCM")}
    y = x
    for k in ("T", "Shr", "CCM"):
        y = torch.clip(torch_ref.process(OPS[k], y, ps[k]), 0.0, 1.0)
    (y * torch.from_numpy(g["grad_out"])).sum().backward()
    assert_scaled(x.grad.numpy(), g["chain.x"], 1e-6)
    for k in ("T", "Shr", "CCM"):
        assert_scaled(ps[k].grad.numpy(), g[f"chain.{k}"], 1e-5)


def test_breakpoint_and_tie_pixels_carry_both_conventions(golden):
    """Row 2 of the image holds x = i/8: torch.clamp's closed interval gives such a pixel the slope of both adjacent tone
    segments, which an open-interval kernel would miss by O(1)."""
    g = golden("filters_imggrad")
    p = g["T.param"][0]
    s = 8.0 / (float(p.sum()) + 1e-30)
    x, go = g["img"][0, 0, 2, 1:7], g["grad_out"][0, 0, 2, 1:7]
    assert np.allclose(x, np.arange(1, 7) / 8.0)
    both = np.array([p[i - 1] + p[i] for i in range(1, 7)]) * s * go
    assert np.allclose(g["T.process"][0, 0, 2, 1:7], both, rtol=1e-5, atol=1e-6)
    assert math.isfinite(float(g["Sp.process"][0, :, 0, 2:5].sum()))
