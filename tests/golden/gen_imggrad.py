#!/usr/bin/env python3
"""Golden image gradients: autograd of the REFERENCE's filters with respect to the input image (d out / d img), written
to tests/golden/filters_imggrad.npz. Same reference import, test image and MKL branch as gen_golden.py; runs only in the
build container (the reference never travels to the GPU box).

    python tests/golden/gen_imggrad.py [--out DIR]

Contents (`key` = the filters.npz key of a filter: E, G, CCM, Shr, NLM, T, Ct, Sp, BW, W, USM, ShrV2, C):
  img, grad_out                  the 13-filter case: filters.npz's image and filters_grad.npz's grad_out draw
  {key}.param                    the parameters of filters.npz / filters_grad.npz
  {key}.process / {key}.forward  x.grad of sum(process(x) * G) and of sum(clip(process(x), 0, 1) * G)
  nlm.{tag}.img / .h / .grad_out / .process / .forward
                                 NLM wrap-around cases: nlm.npz's `a` and `odd`, and `const` (a constant 5x9 patch: the
                                 patch distance is 0 at non-zero offsets)
  chain.*                        clip(CCM(clip(Shr(clip(T(x)))))): x.grad and the three parameter gradients
"""
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
import gen_golden  # noqa: E402  (sets MKL_CBWR=COMPATIBLE before numpy / torch load)
from gen_golden import import_reference, test_image  # noqa: E402

import numpy as np  # noqa: E402
import torch  # noqa: E402

KEYS = [("E", "ExposureFilter"), ("G", "GammaFilter"), ("CCM", "CCMFilter"), ("Shr", "SharpenFilter"),
        ("NLM", "DenoiseFilter"), ("T", "ToneFilter"), ("Ct", "ContrastFilter"), ("Sp", "SaturationPlusFilter"),
        ("BW", "WNBFilter"), ("W", "ImprovedWhiteBalanceFilter"), ("USM", "SharpenUSMFilter"),
        ("ShrV2", "SharpenFilterV2"), ("C", "ColorFilter")]


def _param(f, key, golden):
    # ToneFilter / ColorFilter.process take the regressor's 5-d layout (as gen_golden.py's parameter-gradient fixture)
    if key in ("T", "C"):
        return f.filter_param_regressor(torch.from_numpy(golden[f"{key}.feat"])).detach()
    return torch.from_numpy(golden[f"{key}.param"]).clone()


def _img_grad(fn, x, G, clip):
    x = torch.from_numpy(x).clone().requires_grad_(True)
    y = fn(x)
    if clip:
        y = torch.clip(y, 0.0, 1.0)
    (y * torch.from_numpy(G)).sum().backward()
    return x.grad.numpy().copy()


def main(out_dir):
    import warnings
    warnings.filterwarnings("ignore")
    torch.set_num_threads(4)
    filters, cfg, _, _ = import_reference()
    fl = np.load(os.path.join(HERE, "filters.npz"))
    out = {}

    # ---------------------------------------------------------------- the 13 filters on the edge-case test image
    img = test_image(2, 24, 40, seed=11)
    assert np.array_equal(img, fl["img"])
    G = np.random.default_rng(6).normal(0.0, 1.0, img.shape).astype(np.float32)   # filters_grad.npz's draw
    out["img"], out["grad_out"] = img, G
    for key, cls in KEYS:
        f = getattr(filters, cls)(cfg, predict=False)
        p = _param(f, key, fl)
        out[f"{key}.param"] = p.reshape(2, -1).numpy()
        for mode in ("process", "forward"):
            out[f"{key}.{mode}"] = _img_grad(lambda x: f.process(x, p), img, G, mode == "forward")

    # ---------------------------------------------------------------- NLM: circular wrap, D == 0 away from the zero offset
    nlm = filters.DenoiseFilter(cfg, predict=False)
    cases = []
    for tag, shape, hs, seed in (("a", (2, 20, 28), [0.08, 0.5], 21), ("odd", (1, 37, 70), [0.02], 23)):
        x = test_image(shape[0], shape[1], shape[2], seed=seed, special=False)     # nlm.npz's images
        x += np.random.default_rng(seed).normal(0, 0.02, x.shape).astype(np.float32)
        cases.append((tag, x, hs, seed))
    x = test_image(1, 16, 24, seed=24, special=False)
    x += np.random.default_rng(24).normal(0, 0.02, x.shape).astype(np.float32)
    x[:, :, 4:9, 6:15] = np.float32(0.375)
    cases.append(("const", x, [0.3], 24))
    for tag, x, hs, seed in cases:
        h = np.asarray(hs, np.float32).reshape(-1, 1)
        g = np.random.default_rng(100 + seed).normal(0.0, 1.0, x.shape).astype(np.float32)
        out[f"nlm.{tag}.img"], out[f"nlm.{tag}.h"], out[f"nlm.{tag}.grad_out"] = x, h, g
        for mode in ("process", "forward"):
            out[f"nlm.{tag}.{mode}"] = _img_grad(lambda t: nlm.process(t, torch.from_numpy(h)), x, g, mode == "forward")

    # ---------------------------------------------------------------- one chain: Tone -> Sharpen -> CCM (Filter.forward's clip)
    fT, fS, fC = filters.ToneFilter(cfg), filters.SharpenFilter(cfg), filters.CCMFilter(cfg)
    pT, pS, pC = (_param(fT, "T", fl).requires_grad_(True), _param(fS, "Shr", fl).requires_grad_(True),
                  _param(fC, "CCM", fl).requires_grad_(True))
    x = torch.from_numpy(img).clone().requires_grad_(True)
    y = torch.clip(fT.process(x, pT), 0.0, 1.0)
    y = torch.clip(fS.process(y, pS), 0.0, 1.0)
    y = torch.clip(fC.process(y, pC), 0.0, 1.0)
    (y * torch.from_numpy(G)).sum().backward()
    out["chain.x"] = x.grad.numpy().copy()
    out["chain.T"] = pT.grad.reshape(2, -1).numpy().copy()
    out["chain.Shr"] = pS.grad.reshape(2, -1).numpy().copy()
    out["chain.CCM"] = pC.grad.reshape(2, -1).numpy().copy()
    np.savez_compressed(os.path.join(out_dir, "filters_imggrad.npz"), **out)


if __name__ == "__main__":
    args = sys.argv[1:]
    out_dir = HERE
    if args[:1] == ["--out"]:
        out_dir = os.path.abspath(args[1])
        os.makedirs(out_dir, exist_ok=True)
    elif args:
        raise SystemExit("usage: gen_imggrad.py [--out DIR]")
    gen_golden.OUT = out_dir
    main(out_dir)
