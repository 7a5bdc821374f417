#!/usr/bin/env python3
"""Golden confusion matrices: the REFERENCE's `ConfusionMatrix.process_batch` (yolov3/utils/metrics.py:126-184, the calls
of val_adaptiveisp.py:357,373) on seeded synthetic images, written to tests/golden/confusion.npz. Runs only in the build
container (the reference never travels to the GPU box).

    python tests/golden/gen_confusion.py [--out DIR]

Contents (nc = 5, conf 0.25, IoU 0.45 — the reference's defaults):
  nc, n_images
  det{i} / lab{i} / cm{i}   image i: detections [n,6] (xyxy, conf, class) fp32, labels [m,5] (class, xyxy) fp32, and the
                            [nc+1, nc+1] matrix the reference fills from this image alone (int64). Detections are jittered
                            copies of labels (about 30 % with another class) plus strays; images 0..4 are the empty cases:
                            no labels, no detections, neither, every confidence <= 0.25, labels nothing overlaps.
                            An image with no detections is given as `detections=None` with the label classes (:357), as
                            the evaluation loop does.
  total                     the matrix accumulated over all images in order
  batch.det / batch.offset / batch.targets
                            the same images as one batch: all detections image-major, int32 [n_images + 1] row offsets,
                            and the labels as [n,6] = (image, class, x1, y1, x2, y2)
No two positive IoUs of an image are equal (asserted; the image is redrawn otherwise): the reference leaves ties to numpy's
unstable argsort, so a fixture with ties would pin an accident.
"""
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import matplotlib  # noqa: E402

matplotlib.use("Agg")                     # before the reference's utils import pyplot: no backend switch through the IPython stub
import matplotlib.pyplot  # noqa: E402,F401
import gen_golden  # noqa: E402  (sets MKL_CBWR=COMPATIBLE before numpy loads)

import numpy as np  # noqa: E402
import torch  # noqa: E402

NC, N_RANDOM = 5, 36


def import_reference_metrics(root="/root/reference"):
    gen_golden.import_reference_yolo(os.path.join(root, "yolov3"))
    from utils import metrics
    return metrics


def draw(rs, m, n_near, n_stray, low_conf=False):
    """m labels in a 640 x 480 image, n_near detections jittered around labels, n_stray anywhere."""
    W, H = 640.0, 480.0
    cx, cy = rs.uniform(60, W - 60, m), rs.uniform(60, H - 60, m)
    w, h = rs.uniform(30, 160, m), rs.uniform(30, 160, m)
    lab = np.stack([rs.randint(0, NC, m).astype(np.float64), cx - w / 2, cy - h / 2, cx + w / 2, cy + h / 2], 1).reshape(m, 5)
    rows = []
    for _ in range(n_near if m else 0):
        k = rs.randint(0, m)
        box = lab[k, 1:] + rs.normal(0, 0.06, 4) * np.array([w[k], h[k], w[k], h[k]])
        cls = lab[k, 0] if rs.rand() > 0.3 else float(rs.randint(0, NC))
        rows.append([*box, rs.uniform(0.05, 1.0), cls])
    for _ in range(n_stray):
        x, y = rs.uniform(0, W - 40), rs.uniform(0, H - 40)
        rows.append([x, y, x + rs.uniform(10, 200), y + rs.uniform(10, 200), rs.uniform(0.05, 1.0), float(rs.randint(0, NC))])
    det = np.array(rows, np.float64).reshape(len(rows), 6)
    if len(det):
        det = det[np.argsort(-det[:, 4], kind="stable")]           # post-NMS order: descending confidence
        if low_conf:
            det[:, 4] = np.minimum(det[:, 4] * 0.25, 0.25)
    return det.astype(np.float32), lab.astype(np.float32)


def distinct_ious(metrics, det, lab):
    if not len(det) or not len(lab):
        return True
    iou = metrics.box_iou(torch.from_numpy(lab[:, 1:]), torch.from_numpy(det[:, :4])).numpy().ravel()
    pos = iou[iou > 0]
    return len(np.unique(pos)) == len(pos)


def main(out_dir):
    metrics = import_reference_metrics()
    rs = np.random.RandomState(4242)
    plans = [dict(m=0, n_near=0, n_stray=7), dict(m=6, n_near=0, n_stray=0), dict(m=0, n_near=0, n_stray=0),
             dict(m=5, n_near=9, n_stray=3, low_conf=True), dict(m=4, n_near=0, n_stray=0, far=True)]
    for _ in range(N_RANDOM):
        n = rs.randint(0, 40)
        near = rs.randint(0, n + 1)
        plans.append(dict(m=rs.randint(0, 12), n_near=near, n_stray=n - near))
    out = {"nc": np.array(NC, np.int64), "n_images": np.array(len(plans), np.int64)}
    total = metrics.ConfusionMatrix(NC)
    dets, targets, offsets = [], [], [0]
    for i, plan in enumerate(plans):
        far = plan.pop("far", False)
        while True:
            det, lab = draw(rs, **plan)
            if far:                                                    # detections that overlap no label at all
                det = np.array([[600, 440, 630, 470, 0.9, 1], [1, 1, 9, 9, 0.8, 2]], np.float32)
                lab[:, 1:] = lab[:, 1:] * 0.5 + np.array([100, 100, 100, 100], np.float32)
            if distinct_ious(metrics, det, lab):
                break
        one = metrics.ConfusionMatrix(NC)
        for cm in (one, total):
            if len(det) == 0:
                if len(lab):
                    cm.process_batch(detections=None, labels=torch.from_numpy(lab[:, 0].copy()))
            elif len(lab):
                cm.process_batch(torch.from_numpy(det.copy()), torch.from_numpy(lab.copy()))
        assert np.array_equal(one.matrix, np.rint(one.matrix))
        out[f"det{i}"], out[f"lab{i}"], out[f"cm{i}"] = det, lab, one.matrix.astype(np.int64)
        dets.append(det)
        targets.append(np.concatenate([np.full((len(lab), 1), i, np.float32), lab], 1))
        offsets.append(offsets[-1] + len(det))
    out["total"] = total.matrix.astype(np.int64)
    out["batch.det"] = np.concatenate(dets, 0)
    out["batch.offset"] = np.array(offsets, np.int32)
    out["batch.targets"] = np.concatenate(targets, 0)
    np.savez_compressed(os.path.join(out_dir, "confusion.npz"), **out)
    print(f"confusion.npz: {len(out)} arrays, {len(plans)} images, {offsets[-1]} detections, {len(out['batch.targets'])} labels, "
          f"{int(out['total'].sum())} counts")


if __name__ == "__main__":
    out = HERE
    if "--out" in sys.argv:
        out = sys.argv[sys.argv.index("--out") + 1]
    main(out)
