#!/usr/bin/env python3
"""Golden Bayer sensor: the REFERENCE's `unprocess(rgb, "RGGB")` (isp/unprocess_np.py:217-245, ending in `mosaic` :82-98)
laid out by its `reconstruct_bayer(..., 'rggb')` (:111-128), and its metadata draws, written to tests/golden/bayer.npz.
Runs only in the build container (the reference never travels to the GPU box).

    python tests/golden/gen_bayer.py [--out DIR]

Contents:
  case{k}.img            seeded even-sized uint8 HWC BGR image (0 and 255 present), k = 0..5
  case{k}.seed           np.random.seed(seed) before the call unprocess(img[..., ::-1] / 255, "RGGB")
  case{k}.plane          reconstruct_bayer(packed, 'rggb') of the call's packed output: float64 [H, W]
  case{k}.rgb2cam        random_ccm() after np.random.seed(seed)
  case{k}.gains          (rgb_gain, red_gain, blue_gain): random_gains() after it, the call's own order
  sat.img / .seed / .plane / .rgb2cam / .gains
                         the same for a near-white image, where safe_invert_gains' mask is reached (`unprocess` has no
                         pre-scale, so white stays white)
  cfa.{RGGB,GRBG,GBRG,BGGR}
                         the channel (0 R, 1 G, 2 B) at every pixel of a 4 x 6 image: `mosaic`'s packing of an image
                         whose channel c holds c everywhere, laid out by reconstruct_bayer for that pattern

`unprocess` has no pre-scale, no brightness ratio and no noise: the kernel reproduces it with p[PRESCALE] = 1,
p[RATIO] = 1 and flags UNPROCESS. Before anything is written, tests/_bayerref.py must reproduce every plane to 1e-12.
"""
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
import gen_golden  # noqa: E402,F401  (sets MKL_CBWR=COMPATIBLE before numpy loads)

import numpy as np  # noqa: E402

import _bayerref as R  # noqa: E402
import _unprocessref  # noqa: E402
from gen_unprocess import import_unprocess  # noqa: E402

# (h, w, seed): even sides, at most 32 x 48
CASES = [(2, 2, 10), (4, 6, 11), (8, 2, 12), (16, 10, 13), (32, 48, 14), (6, 48, 15)]


def _call(U, img, seed):
    np.random.seed(seed)
    packed, meta = U.unprocess(img[..., ::-1] / 255.0, "RGGB")
    plane = U.reconstruct_bayer(packed, "rggb")
    np.random.seed(seed)
    rgb2cam = U.random_ccm()
    gains = np.array(U.random_gains(), np.float64)
    assert gains[0] == meta["rgb_gain"] and gains[1] == meta["red_gain"] and gains[2] == meta["blue_gain"]
    assert np.array_equal(np.linalg.inv(rgb2cam), meta["cam2rgb"])
    assert plane.dtype == np.float64 and plane.shape == img.shape[:2]
    err = np.abs(R.sensor_plane(img, rgb2cam, *gains, pattern="RGGB") - plane).max()
    assert err <= 1e-12, err
    return plane, rgb2cam, gains


def main(out_dir):
    U = import_unprocess()
    rs = np.random.RandomState(2025)
    out = {}
    for k, (h, w, seed) in enumerate(CASES):
        img = rs.randint(0, 256, size=(h, w, 3)).astype(np.uint8)
        img.reshape(-1)[0], img.reshape(-1)[-1] = 0, 255
        c = f"case{k}."
        out[c + "img"], out[c + "seed"] = img, np.int64(seed)
        out[c + "plane"], out[c + "rgb2cam"], out[c + "gains"] = _call(U, img, seed)

    sat = rs.randint(250, 256, size=(10, 8, 3)).astype(np.uint8)
    sat[0] = rs.randint(200, 240, size=(8, 3))                   # the first row stays below the inflection
    sat[1, 0] = 255
    out["sat.img"], out["sat.seed"] = sat, np.int64(8)
    out["sat.plane"], out["sat.rgb2cam"], out["sat.gains"] = _call(U, sat, 8)
    assert (_unprocessref.saturation_mask(sat, out["sat.rgb2cam"]) > 0.05).sum() >= 10

    label = np.zeros((4, 6, 3))
    label[..., 1], label[..., 2] = 1, 2
    for name in R.CFA:
        out["cfa." + name] = U.reconstruct_bayer(U.mosaic(label, "RGGB"), name.lower()).astype(np.int64)
    np.savez_compressed(os.path.join(out_dir, "bayer.npz"), **out)
    print(f"wrote {os.path.join(out_dir, 'bayer.npz')} ({len(out)} arrays)")


if __name__ == "__main__":
    args = sys.argv[1:]
    if args[:1] == ["--out"]:
        main(args[1])
    elif not args:
        main(HERE)
    else:
        raise SystemExit("usage: gen_bayer.py [--out DIR]")
