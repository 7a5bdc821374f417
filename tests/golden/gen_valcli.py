#!/usr/bin/env python3
"""Golden outputs of the evaluation CLI's host writers: the REFERENCE's `save_one_txt` / `save_one_json`
(yolov3/val_adaptiveisp.py:56-76) and the array its `save_img` (util.py:21-40) hands to cv2.imwrite, written to
tests/golden/valcli.npz. Runs only in the build container (the reference never travels to the GPU box); cv2 is absent and
stubbed: cvtColor(RGB2BGR) is the channel swap it is, imwrite records its argument.

    python tests/golden/gen_valcli.py [--out DIR]

Contents:
  class_map               coco80_to_coco91_class()
  case.names              the case names below (space separated)
  (every text below is stored as its UTF-8 bytes, a uint8 array)
  <case>.predn / .shape / .path
                          native-space detections [n,6] (xyxy, conf, class) fp32, the native (h, w), the image path
  <case>.txt / .txt_conf  the file save_one_txt(predn, save_conf, shape, file) leaves behind (save_conf False / True)
  <case>.json             json.dumps of the list save_one_json(predn, [], Path(path), class_map) appends
  img{k} / saved{k}       fp32 CHW RGB input of save_img(img, 'x/name.png', dir, None, 'CHW', False) and the HWC BGR
                          float32 array it passes to cv2.imwrite (before OpenCV's float -> 8U conversion)
"""
import contextlib
import io
import json
import os
import sys
import tempfile
from pathlib import Path

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import gen_golden  # noqa: E402  (sets MKL_CBWR=COMPATIBLE before numpy loads)

import numpy as np  # noqa: E402
import torch  # noqa: E402

CASES = [("numeric", "/data/images/000000397133.jpg", (427, 640), 7, 80),
         ("named", "/data/images/night_street-1.png", (720, 1280), 11, 7),
         ("zeros", "/data/images/0042.png", (375, 500), 3, 80),
         ("empty", "/data/images/2.png", (512, 384), 0, 80)]


def import_reference_val(root="/root/reference"):
    gen_golden.import_reference(root)
    gen_golden.import_reference_yolo(os.path.join(root, "yolov3"))
    sys.path.insert(0, root)
    with contextlib.redirect_stdout(io.StringIO()), contextlib.redirect_stderr(io.StringIO()):
        import val_adaptiveisp
    return val_adaptiveisp


def predictions(rs, n, nc, shape, zeros=False):
    h0, w0 = shape
    x1 = rs.uniform(-5, w0 * 0.9, n)
    y1 = rs.uniform(-5, h0 * 0.9, n)
    x2 = x1 + rs.uniform(0.01, w0 * 0.5, n)
    y2 = y1 + rs.uniform(0.01, h0 * 0.5, n)
    conf = rs.uniform(0.001, 1.0, n)
    conf[:2] = (0.00123456789, 0.5)[:min(n, 2)]
    cls = rs.randint(0, nc, n)
    p = np.stack([x1, y1, x2, y2, conf, cls], 1).astype(np.float32).reshape(n, 6)
    if zeros and n:
        p[0, :4] = (0.0, 0.0, float(w0), float(h0))                       # a whole-image box, exact integers
    return p


def tie_values():
    """fp32 x in (0, 1) with x * 255.0f exactly k + 0.5 (ties of the float -> 8U rounding), for as many k as exist."""
    out = []
    for k in range(255):
        c = np.float32((k + 0.5) / 255.0)
        for d in range(-4, 5):
            v = np.float32(c + np.float32(d) * np.spacing(c))
            if np.float32(v * np.float32(255.0)) == np.float32(k + 0.5):
                out.append(v)
                break
    return np.array(out, np.float32)


def save_img_inputs():
    rs = np.random.RandomState(7)
    ties = tie_values()
    special = np.array([np.nan, np.inf, -np.inf, -0.0, 0.0, -1e-30, 1e-30, -3.5, 7.25, 1.0, np.nextafter(np.float32(1), 2),
                        np.float32(0.5) / 255, np.float32(1.5) / 255, np.float32(254.5) / 255], np.float32)
    imgs = []
    a = np.concatenate([special, ties, rs.uniform(-0.2, 1.2, 3 * 9 * 17 - len(special) - len(ties))]).astype(np.float32)
    imgs.append(rs.permutation(a).reshape(3, 9, 17))
    imgs.append(np.array([np.nan, 2.0, -np.inf], np.float32).reshape(3, 1, 1))
    imgs.append(rs.uniform(0, 1, (3, 4, 5)).astype(np.float32))
    return imgs, ties


def text(s):
    """Text as UTF-8 bytes (a uint8 array: numeric, so tools/regen_check.sh compares it like every other array)."""
    return np.frombuffer(s.encode("utf-8"), np.uint8).copy()


def main(out_dir):
    v = import_reference_val()
    out = {"class_map": np.array(v.coco80_to_coco91_class(), np.int64)}
    rs = np.random.RandomState(2025)
    names = []
    with tempfile.TemporaryDirectory() as tmp:
        for name, path, shape, n, nc in CASES:
            names.append(name)
            p = predictions(rs, n, nc, shape, zeros=(name == "zeros"))
            out[f"{name}.predn"], out[f"{name}.shape"], out[f"{name}.path"] = p, np.array(shape, np.int64), text(path)
            for key, conf in (("txt", False), ("txt_conf", True)):
                f = Path(tmp) / f"{name}_{key}.txt"
                v.save_one_txt(torch.from_numpy(p), conf, shape, file=f)
                out[f"{name}.{key}"] = text(f.read_text() if f.exists() else "")
            jdict = []
            v.save_one_json(torch.from_numpy(p), jdict, Path(path), v.coco80_to_coco91_class())
            out[f"{name}.json"] = text(json.dumps(jdict))
        out["case.names"] = text(" ".join(names))

        # save_img: the array cv2.imwrite receives
        saved = []

        class _CV2:
            COLOR_RGB2BGR = 4

            @staticmethod
            def cvtColor(img, code):
                assert code == _CV2.COLOR_RGB2BGR
                return img[..., ::-1]

            @staticmethod
            def imwrite(path, arr):
                saved.append(np.array(arr, copy=True))
                return True

        v.save_img.__globals__["cv2"] = _CV2
        imgs, ties = save_img_inputs()
        for k, im in enumerate(imgs):
            v.save_img(torch.from_numpy(im.copy()), f"x/name{k}.png", tmp, None, "CHW", False)
            assert saved[-1].dtype == np.float32, saved[-1].dtype
            out[f"img{k}"], out[f"saved{k}"] = im, saved[-1]
        out["ties"] = ties
    np.savez_compressed(os.path.join(out_dir, "valcli.npz"), **out)
    print(f"valcli.npz: {len(out)} arrays, {len(ties)} tie values")


if __name__ == "__main__":
    out = HERE
    if "--out" in sys.argv:
        out = sys.argv[sys.argv.index("--out") + 1]
    main(out)
