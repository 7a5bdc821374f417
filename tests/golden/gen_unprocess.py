#!/usr/bin/env python3
"""Golden unprocess: the REFERENCE's `unprocess_wo_mosaic` (isp/unprocess_np.py:248-292) and its metadata draws, written to
tests/golden/unprocess.npz. Runs only in the build container (the reference never travels to the GPU box).

    python tests/golden/gen_unprocess.py [--out DIR]

Contents:
  img{i}                 seeded uint8 HWC BGR images (odd sizes, 0 and 255 present), i = 0..3
  case{k}.img / .seed / .add_noise / .bri (NaN NaN: None) / .noise_level (NaN: None) / .use_linear
                         the call: unprocess_wo_mosaic(img{i}[..., ::-1] / 255, add_noise, bri, noise_level, use_linear)
                         after np.random.seed(seed), as dataset.py:458-471 calls it
  case{k}.rgb2cam        random_ccm() after np.random.seed(seed)
  case{k}.gains          (rgb_gain, red_gain, blue_gain) of the metadata;  case{k}.gain, case{k}.noise = (shot, read)
  case{k}.out            the NOISE-FREE output: the same call under the same seed with add_noise=False (float64 HWC RGB)
  sat.img / .rgb2cam / .gains / .out
                         the saturation-mask case: inverse_smoothstep -> gamma_expansion -> apply_ccm -> safe_invert_gains
                         -> clip at pre-scale 1.0 on near-white pixels (unprocess_wo_mosaic's x 0.9 caps white at ~0.62
                         after the gamma expansion, so its own cases never reach the mask)
"""
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import gen_golden  # noqa: E402,F401  (sets MKL_CBWR=COMPATIBLE before numpy loads)

import numpy as np  # noqa: E402

SIZES = [(7, 9), (13, 5), (1, 1), (4, 11)]
# (image, seed, add_noise, brightness_range, noise_level, use_linear)
CASES = [(0, 0, False, None, None, False),
         (1, 1, True, None, None, False),
         (2, 2, True, None, None, True),
         (3, 3, True, (0.1, 0.3), None, False),
         (0, 4, True, (0.1, 0.3), 0.005, False),
         (1, 5, True, None, 0.002, True),
         (2, 6, False, (0.2, 0.5), None, False),
         (3, 7, False, None, None, True)]


def import_unprocess(root="/root/reference"):
    import matplotlib
    matplotlib.use("Agg")
    sys.path.insert(0, root)
    from isp import unprocess_np
    return unprocess_np


def test_images():
    rs = np.random.RandomState(2024)
    out = []
    for i, (h, w) in enumerate(SIZES):
        im = rs.randint(0, 256, size=(h, w, 3)).astype(np.uint8)
        im.reshape(-1)[0] = 0
        im.reshape(-1)[-1] = 255
        out.append(im)
    return out


def main(out_dir):
    U = import_unprocess()
    imgs = test_images()
    out = {f"img{i}": im for i, im in enumerate(imgs)}
    for k, (i, seed, noise, bri, level, lin) in enumerate(CASES):
        rgb = imgs[i][..., ::-1] / 255.0
        np.random.seed(seed)
        _, meta = U.unprocess_wo_mosaic(rgb, noise, bri, level, lin)
        np.random.seed(seed)
        rgb2cam = U.random_ccm()
        np.random.seed(seed)
        clean, meta0 = U.unprocess_wo_mosaic(rgb, False, bri, level, lin)
        assert meta0["gain"] == meta["gain"] and meta0["rgb_gain"] == meta["rgb_gain"]
        c = f"case{k}."
        out[c + "img"], out[c + "seed"] = np.int64(i), np.int64(seed)
        out[c + "add_noise"], out[c + "use_linear"] = np.bool_(noise), np.bool_(lin)
        out[c + "bri"] = np.array(bri if bri is not None else (np.nan, np.nan), np.float64)
        out[c + "noise_level"] = np.float64(level if level is not None else np.nan)
        out[c + "rgb2cam"] = rgb2cam
        out[c + "gains"] = np.array([meta["rgb_gain"], meta["red_gain"], meta["blue_gain"]], np.float64)
        out[c + "gain"] = np.float64(meta["gain"])
        out[c + "noise"] = np.array(meta["noise"], np.float64)
        out[c + "out"] = clean

    rs = np.random.RandomState(99)
    sat = rs.randint(250, 256, size=(9, 7, 3)).astype(np.uint8)
    sat[0] = rs.randint(200, 240, size=(7, 3))                   # the first row stays below the inflection
    sat[1, 0] = 255
    np.random.seed(8)
    rgb2cam = U.random_ccm()
    gains = U.random_gains()
    x = U.inverse_smoothstep(sat[..., ::-1] / 255.0)
    x = U.gamma_expansion(x)
    x = U.apply_ccm(x, rgb2cam)
    x = U.safe_invert_gains(x, *gains)
    out["sat.img"], out["sat.rgb2cam"], out["sat.gains"] = sat, rgb2cam, np.array(gains, np.float64)
    out["sat.out"] = np.clip(x, 0.0, 1.0)
    np.savez_compressed(os.path.join(out_dir, "unprocess.npz"), **out)
    print(f"wrote {os.path.join(out_dir, 'unprocess.npz')} ({len(out)} arrays)")


if __name__ == "__main__":
    args = sys.argv[1:]
    if args[:1] == ["--out"]:
        main(args[1])
    elif not args:
        main(HERE)
    else:
        raise SystemExit("usage: gen_unprocess.py [--out DIR]")
