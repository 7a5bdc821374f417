#!/usr/bin/env python3
"""Fixture generator for the training augmentation: imports the REFERENCE's utils/augmentations.py and utils/general.py
unmodified (absent third-party modules stubbed, as gen_golden.py does) and records, per case, what `random_perspective`,
the table construction of `augment_hsv`, `xyxy2xywhn(clip=True, eps=1e-3)` and the two flips make of seeded draws and a
label set: tests/golden/augment.npz. No pixel is computed: the cv2 stand-in has `getRotationMatrix2D` as its closed form,
a `warpAffine` that records the matrix it is given and returns a blank frame, and colour functions that record the tables.

Runs only where the reference is checked out (no GPU needed); the fixture it writes is committed next to it.

    python tests/golden/gen_augment.py [--out DIR]
"""
import math
import os
import random
import sys
import types

import numpy as np

sys.dont_write_bytecode = True
HERE = os.path.dirname(os.path.abspath(__file__))

# (name, S, seed, hyp, labels in: class x y w h normalised to the frame)
LOW = dict(hsv_h=0.015, hsv_s=0.7, hsv_v=0.4, degrees=0.0, translate=0.1, scale=0.5, shear=0.0, perspective=0.0,
           flipud=0.0, fliplr=0.5)
KEYS = ("hsv_h", "hsv_s", "hsv_v", "degrees", "translate", "scale", "shear", "perspective", "flipud", "fliplr")
STRONG = dict(LOW, degrees=10.0, shear=5.0, scale=0.5, translate=0.1, flipud=0.5)
BOXES = [[3, 0.50, 0.50, 0.30, 0.20], [7, 0.25, 0.30, 0.10, 0.40], [0, 0.70, 0.75, 0.20, 0.20], [11, 0.40, 0.60, 0.55, 0.35]]
REJECTED = [[1, 0.50, 0.50, 0.004, 0.30],      # under 2 px wide after the warp
            [2, 0.985, 0.50, 0.03, 0.30],      # at the right edge: under 2 px wide after the clip at 64, kept at 416
            [4, 0.50, 0.50, 0.90, 0.008],      # aspect over 100
            [5, 0.50, 0.50, 0.25, 0.25]]       # kept
LEAVING = [[6, 0.04, 0.05, 0.16, 0.12], [8, 0.97, 0.95, 0.20, 0.22], [9, 0.50, 0.02, 0.30, 0.10]]
# a 5 x 5 grid under a translation of up to 0.45 of the frame: boxes leave it whole, and with seed 40 one keeps a sliver over
# 2 px a side with under a tenth of its area (rejected by the area ratio alone)
GRID = [[5 * i + j, (i + 0.5) / 5, (j + 0.5) / 5, 0.16, 0.16] for i in range(5) for j in range(5)]
CASES = []
for S in (64, 416):
    for k in range(3):
        CASES.append((f"low_{S}_{k}", S, 10 + k, LOW, BOXES))
        CASES.append((f"strong_{S}_{k}", S, 20 + k, STRONG, BOXES))
    CASES.append((f"rejected_{S}", S, 30, dict(LOW, scale=0.05, translate=0.0, fliplr=0.0), REJECTED))
    CASES.append((f"leaving_{S}", S, 31, STRONG, LEAVING))
    CASES.append((f"arearatio_{S}", S, 40, dict(LOW, scale=0.0, translate=0.45, fliplr=0.0), GRID))
    CASES.append((f"empty_{S}", S, 32, STRONG, []))
    CASES.append((f"nohsv_{S}", S, 33, dict(STRONG, hsv_h=0.0, hsv_s=0.0, hsv_v=0.0), BOXES))


class _AnyObj:
    def __init__(self, *a, **k): pass
    def __call__(self, *a, **k): return _AnyObj()
    def __getattr__(self, n):
        if n.startswith("__"):
            raise AttributeError(n)
        return _AnyObj()
    def __mro_entries__(self, bases): return (object,)


class _AnyModule(types.ModuleType):
    def __getattr__(self, name):
        if name.startswith("__"):
            raise AttributeError(name)
        return _AnyObj()


class _Cv2(types.ModuleType):
    """What random_perspective and augment_hsv call, without pixels."""
    COLOR_BGR2HSV, COLOR_HSV2BGR = 40, 54

    def __init__(self):
        super().__init__("cv2")
        self.matrices, self.tables = [], []

    def __getattr__(self, name):
        if name.startswith("__"):
            raise AttributeError(name)
        return _AnyObj()

    @staticmethod
    def getRotationMatrix2D(angle, center, scale):
        a = angle * math.pi / 180
        alpha, beta = scale * math.cos(a), scale * math.sin(a)
        cx, cy = center
        return np.array([[alpha, beta, (1 - alpha) * cx - beta * cy], [-beta, alpha, beta * cx + (1 - alpha) * cy]])

    def warpAffine(self, im, M, dsize, borderValue=None):
        self.matrices.append(np.array(M, np.float64))
        return np.zeros((dsize[1], dsize[0], 3), im.dtype)

    def cvtColor(self, im, code, dst=None):
        return im

    def split(self, im):
        return [im[..., c] for c in range(3)]

    def LUT(self, plane, table):
        self.tables.append(np.array(table))
        return plane

    def merge(self, planes):
        return np.stack(planes, axis=-1)


def import_reference(root="/root/reference/yolov3"):
    cv2 = _Cv2()
    sys.modules["cv2"] = cv2
    for n in ["seaborn", "thop", "ultralytics", "ultralytics.utils", "ultralytics.utils.plotting", "ultralytics.utils.checks",
              "torchvision", "torchvision.ops", "torchvision.datasets", "torchvision.transforms",
              "torchvision.transforms.functional", "IPython", "IPython.display", "pandas", "pkg_resources", "matplotlib",
              "matplotlib.pyplot", "PIL", "PIL.Image", "PIL.ImageDraw", "PIL.ImageFont", "scipy", "scipy.signal", "requests"]:
        try:
            __import__(n)
        except Exception:
            m = _AnyModule(n)
            m.__path__ = []
            sys.modules[n] = m
    sys.path.insert(0, root)
    from utils import augmentations, general
    return cv2, augmentations, general


def main(out_dir=HERE):
    cv2, A, G = import_reference()
    # numeric arrays only: the case names as the bytes of one newline-joined string, the hyper-parameters in KEYS' order
    out = {"names": np.frombuffer("\n".join(c[0] for c in CASES).encode(), np.uint8)}
    for name, S, seed, hyp, rows in CASES:
        random.seed(seed)
        np.random.seed(seed)
        lb = np.array(rows, np.float64).reshape(-1, 5)
        targets = lb.copy()
        if len(lb):
            targets[:, 1:] = G.xywhn2xyxy(lb[:, 1:], S, S, padw=0, padh=0)
        cv2.matrices.clear()
        cv2.tables.clear()
        frame = np.zeros((S, S, 3), np.uint8)
        # the uniform draw of the scale is the fourth of random_perspective's eight: read it back from a twin generator
        twin = random.Random(seed)
        for _ in range(3):
            twin.uniform(0, 1)
        s = twin.uniform(1 - hyp["scale"], 1 + hyp["scale"])
        _, warped = A.random_perspective(frame, targets.copy(), degrees=hyp["degrees"], translate=hyp["translate"],
                                         scale=hyp["scale"], shear=hyp["shear"], perspective=hyp["perspective"])
        M = np.eye(3)
        if cv2.matrices:                                           # no call for an identity draw
            M[:2] = cv2.matrices[0]
        labels = np.array(warped, np.float64).reshape(-1, 5)
        if len(labels):
            labels[:, 1:5] = G.xyxy2xywhn(labels[:, 1:5], w=S, h=S, clip=True, eps=1E-3)
        A.augment_hsv(frame, hgain=hyp["hsv_h"], sgain=hyp["hsv_s"], vgain=hyp["hsv_v"])
        luts = np.stack(cv2.tables).astype(np.uint8) if cv2.tables else np.zeros((0, 256), np.uint8)
        flipud = random.random() < hyp["flipud"]
        if flipud and len(labels):
            labels[:, 2] = 1 - labels[:, 2]
        fliplr = random.random() < hyp["fliplr"]
        if fliplr and len(labels):
            labels[:, 1] = 1 - labels[:, 1]
        out[f"{name}/S"], out[f"{name}/seed"] = np.int64(S), np.int64(seed)
        out[f"{name}/hyp_values"] = np.array([hyp[k] for k in KEYS], np.float64)
        out[f"{name}/labels_in"], out[f"{name}/labels_out"] = lb, labels
        out[f"{name}/M"], out[f"{name}/s"], out[f"{name}/luts"] = M, np.float64(s), luts
        out[f"{name}/flips"] = np.array([flipud, fliplr])
        print(f"{name}: {len(lb)} -> {len(labels)} labels, s = {s:.4f}, flips {flipud} {fliplr}, {len(luts)} tables")
    path = os.path.join(out_dir, "augment.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main(sys.argv[sys.argv.index("--out") + 1] if "--out" in sys.argv else HERE)
