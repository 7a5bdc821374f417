"""Host-side outputs of the evaluation CLI (python -m adaptiveisp_amd.val), in the reference's formats
(yolov3/val_adaptiveisp.py:56-76, util.py:21-40):

  save_one_txt    labels/<stem>.txt: one `class x y w h [conf]` row per detection, xywh normalised to the native image,
                  every number printed with '%g'
  save_one_json   COCO-JSON records {image_id, category_id, bbox (top-left xywh, 3 decimals), score (5 decimals)}; the
                  category is the COCO paper id of the 80-class index, as the reference maps every dataset (is_coco is
                  always True there, :201)
  ImageWriter     the per-step retouched images: uint8 BGR arrays from adaisp_export_u8, encoded by PIL on a small thread
                  pool in the format the file extension names

The box arithmetic is fp32, element for element what the reference's torch code does, so the text is byte-equal to
its output (pinned by tests/golden/valcli.npz).
"""
import os
from collections import deque
from concurrent.futures import ThreadPoolExecutor
from pathlib import Path

import numpy as np
import torch

# COCO's 91 category ids minus the 11 that the 2014/2017 annotations never use (12, 26, 29, 30, 45, 66, 68, 69, 71, 83, 91):
# index k of an 80-class detector -> its COCO category id
_COCO_UNUSED = (12, 26, 29, 30, 45, 66, 68, 69, 71, 83, 91)


def coco80_to_coco91_class():
    return [i for i in range(1, 92) if i not in _COCO_UNUSED]


def _center_xywh(predn):
    """predn [n,>=4] xyxy -> fp32 (cx, cy, w, h) columns."""
    b = predn[:, :4].to(torch.float32)
    return (b[:, 0] + b[:, 2]) / 2, (b[:, 1] + b[:, 3]) / 2, b[:, 2] - b[:, 0], b[:, 3] - b[:, 1]


def txt_rows(predn, save_conf, shape):
    """The lines save_one_txt appends for one image: predn [n,6] (xyxy in native pixels, conf, class), shape (h0, w0)."""
    predn = torch.as_tensor(predn, dtype=torch.float32).reshape(-1, 6)
    h0, w0 = (int(v) for v in shape)
    cx, cy, w, h = _center_xywh(predn)
    # division by the integer size in fp32, as a float32 tensor over an int64 one
    xywh = torch.stack((cx / w0, cy / h0, w / w0, h / h0), 1).tolist()
    rows = []
    for (conf, cls), box in zip(predn[:, 4:6].tolist(), xywh):
        vals = (cls, *box, conf) if save_conf else (cls, *box)
        rows.append(" ".join("%g" % v for v in vals) + "\n")
    return rows


def save_one_txt(predn, save_conf, shape, file):
    rows = txt_rows(predn, save_conf, shape)
    with open(file, "a") as f:
        f.write("".join(rows))


def image_id(path):
    stem = Path(path).stem
    return int(stem) if stem.isnumeric() else stem


def save_one_json(predn, jdict, path, class_map):
    """Appends one record per detection of the image at `path` to the list `jdict`."""
    predn = torch.as_tensor(predn, dtype=torch.float32).reshape(-1, 6)
    iid = image_id(path)
    cx, cy, w, h = _center_xywh(predn)
    boxes = torch.stack((cx - w / 2, cy - h / 2, w, h), 1).tolist()
    for (conf, cls), box in zip(predn[:, 4:6].tolist(), boxes):
        jdict.append({"image_id": iid, "category_id": class_map[int(cls)], "bbox": [round(v, 3) for v in box],
                      "score": round(conf, 5)})


def encode_image(path, bgr):
    """Writes HWC uint8 BGR `bgr` to `path` in the format its extension names: PNG / BMP / TIFF / WebP lossless, JPEG at
    quality 95 (cv2.imwrite's default)."""
    from PIL import Image
    im = Image.fromarray(bgr[:, :, ::-1].copy())
    ext = os.path.splitext(path)[1].lower()
    if ext in (".jpg", ".jpeg"):
        im.save(path, quality=95)
    elif ext == ".webp":
        im.save(path, lossless=True)
    else:
        im.save(path)


class ImageWriter:
    """Encodes images on `workers` threads. submit() hands over an array the caller no longer touches; at most `depth`
    images wait (submit blocks on the oldest beyond that, which bounds the pinned memory held); close() waits for every
    write and re-raises the first failure (`raise_errors=False`: only waits, for a caller that is already unwinding from an
    error of its own)."""

    def __init__(self, workers=4, depth=64):
        self._pool = ThreadPoolExecutor(max_workers=int(workers))
        self._pending = deque()
        self._depth = int(depth)

    def submit(self, path, bgr):
        while len(self._pending) >= self._depth:
            self._pending.popleft().result()
        self._pending.append(self._pool.submit(encode_image, path, bgr))

    def close(self, raise_errors=True):
        if self._pool is None:
            return
        self._pool.shutdown(wait=True)
        self._pool = None
        first = None
        while self._pending:
            e = self._pending.popleft().exception()
            first = first or e
        if first is not None and raise_errors:
            raise first


def save_confusion_csv(matrix, names, file):
    """confusion_matrix.csv: a header row (`predicted/true`, the class names, `background`), then one row per predicted
    class and the `background` row (missed labels), integer counts. `names`: {class id: name} or a sequence; a class
    without a name is written as its number."""
    matrix = np.asarray(matrix)
    nc = matrix.shape[0] - 1
    get = names.get if isinstance(names, dict) else (lambda c, d: names[c] if c < len(names) else d)
    cols = [str(get(c, str(c))).replace(",", " ") for c in range(nc)] + ["background"]
    with open(file, "w") as f:
        f.write(",".join(["predicted/true"] + cols) + "\n")
        for name, row in zip(cols, matrix):
            f.write(",".join([name] + [str(int(v)) for v in row]) + "\n")
