"""adayolo_match on the MI355X: the matching of a whole batch in one launch (csrc/yolo_match.hip) against the host path.

The yardstick is the host path on CPU fp32 tensors, per image: scale_boxes + xywh2xyxy + process_batch + ConfusionMatrix
(val/boxes.py, val/metrics.py) — the functions tests/golden/evalharness.npz and confusion.npz pin to the reference. The
kernel runs the same fp32 operations in the same order, so `correct` and the confusion matrix must be EQUAL and `predn`
BIT-EQUAL: no tolerance anywhere in this file. `iouv` is made on the device, as the harness makes it, and the yardstick gets
`.cpu()` of that very tensor.

Sizes come from the kernel's two constants (csrc/yolo_match.hip): THREADS = kMatchThreads = 256 detections per round of a
workgroup, CHUNK = kLabelChunk = 256 labels staged in LDS at a time. The large case has THREADS + 44 detections and
2 * CHUNK + 7 labels in one image (a second round, three label chunks, the last one partial); every other case is as small as
its code path allows."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden")
THREADS, CHUNK = 256, 256                                   # kMatchThreads, kLabelChunk
NET = (512, 512)
GEOMS = {"unit": (1.0, 0.0, 0.0, 512, 512),                 # gain 1, no padding
         "pad_x": (0.512, 102.4, 0.0, 1000, 600),           # a 1000 x 600 (h x w) image in 512 x 512: gain < 1, padding on x only
         "pad_y": (0.512, 0.0, 102.4, 600, 1000)}           # 600 x 1000: padding on y only


def _iouv(T):
    return torch.linspace(0.5, 0.95, 10, device=DEV)[:T].contiguous()


def _yardstick(det, offset, targets, geom, iouv, nc, native=False, cm=None, conf=0.25, iou_thres=0.45):
    """The host path per image on CPU fp32 tensors -> (predn [K,6], correct bool [K,T], confusion matrix)."""
    from adaptiveisp_amd.val import ConfusionMatrix, process_batch, scale_boxes, xywh2xyxy
    det, targets = torch.as_tensor(det, dtype=torch.float32), torch.as_tensor(targets, dtype=torch.float32).reshape(-1, 6)
    cm = cm or ConfusionMatrix(nc, conf, iou_thres)
    predn_all, correct_all = [], []
    for b in range(len(offset) - 1):
        pred = det[offset[b]:offset[b + 1]]
        labels = targets[targets[:, 0] == b, 1:]
        nl, npr = labels.shape[0], pred.shape[0]
        correct = torch.zeros(npr, iouv.numel(), dtype=torch.bool)
        predn = pred.clone()
        if not native:
            gain, px, py, h0, w0 = geom[b]
            ratio_pad = ((float(np.float32(gain)),) * 2, (float(np.float32(px)), float(np.float32(py))))
            scale_boxes(NET, predn[:, :4], (int(h0), int(w0)), ratio_pad)
        if npr == 0:
            if nl:
                cm.process_batch(None, labels[:, 0])
        elif nl:
            tbox = labels[:, 1:5].clone() if native else scale_boxes(NET, xywh2xyxy(labels[:, 1:5]), (int(h0), int(w0)), ratio_pad)
            labelsn = torch.cat((labels[:, 0:1], tbox), 1)
            correct = process_batch(predn, labelsn, iouv)
            cm.process_batch(predn, labelsn)
        predn_all.append(predn)
        correct_all.append(correct)
    return torch.cat(predn_all), torch.cat(correct_all), cm.matrix


def _run(det, offset, targets, geom, iouv, nc, native=False, confusion="new", conf=0.25, iou_thres=0.45):
    from adaptiveisp_amd.val import match_batch
    det = torch.as_tensor(det, dtype=torch.float32).reshape(-1, 6).to(DEV)
    targets = torch.as_tensor(targets, dtype=torch.float32).reshape(-1, 6).to(DEV)
    off = torch.as_tensor(np.asarray(offset), dtype=torch.int32).to(DEV)
    g = None if native else torch.tensor(np.asarray(geom, np.float32).reshape(-1, 5)).to(DEV)
    if isinstance(confusion, str):
        confusion = torch.zeros((nc + 1) * (nc + 1), dtype=torch.int32, device=DEV)
    predn, correct = match_batch(det, off, targets, g, iouv, nc, native=native, confusion=confusion, cm_conf=conf, cm_iou=iou_thres)
    torch.cuda.synchronize()
    return predn.cpu(), correct.cpu(), None if confusion is None else confusion.cpu().numpy().reshape(nc + 1, nc + 1)


def _check(det, offset, targets, geom, nc, T=10, native=False):
    iouv = _iouv(T)
    det = np.asarray(det, np.float32).reshape(-1, 6)
    targets = np.asarray(targets, np.float32).reshape(-1, 6)
    want_predn, want_correct, want_cm = _yardstick(det, offset, targets, geom, iouv.cpu(), nc, native)
    predn, correct, cm = _run(det, offset, targets, geom, iouv, nc, native)
    assert predn.shape == want_predn.shape and correct.shape == want_correct.shape and correct.dtype == torch.uint8
    assert np.array_equal(predn.numpy().view(np.uint32), want_predn.numpy().view(np.uint32)), "predn is not bit-equal"
    assert torch.equal(correct.bool(), want_correct), f"correct differs in rows {(correct.bool() != want_correct).any(1).nonzero().flatten()[:8].tolist()}"
    assert set(np.unique(correct.numpy()).tolist()) <= {0, 1}
    np.testing.assert_array_equal(cm, want_cm)
    return predn, correct.bool(), cm


def _scene(seed, n_lab, n_det, nc, shuffle=False, spread=1.0):
    """Per image n_lab[b] labels (xywh, network pixels; some leave the frame) and n_det[b] detections: most of them jittered
    copies of labels (a third with another class), the rest strays; in descending confidence, as NMS leaves them."""
    rng = np.random.default_rng(seed)
    dets, targets, offset = [], [], [0]
    for b, (m, n) in enumerate(zip(n_lab, n_det)):
        c = rng.uniform(0, NET[0], (m, 2))
        wh = rng.uniform(20, 200, (m, 2)) * spread
        cls = rng.integers(0, nc, m)
        targets.append(np.concatenate([np.full((m, 1), b), cls[:, None], c, wh], 1))
        rows = np.zeros((n, 6))
        for i in range(n):
            if m and rng.random() < 0.8:
                k = rng.integers(0, m)
                box = np.concatenate([c[k] - wh[k] / 2, c[k] + wh[k] / 2]) + rng.normal(0, 0.08, 4) * np.tile(wh[k], 2)
                k_cls = cls[k] if rng.random() > 0.33 else rng.integers(0, nc)
            else:
                xy = rng.uniform(-40, NET[0], 2)
                box, k_cls = np.concatenate([xy, xy + rng.uniform(5, 250, 2)]), rng.integers(0, nc)
            rows[i] = (*box, rng.uniform(0.05, 1.0), k_cls)
        dets.append(rows[np.argsort(-rows[:, 4], kind="stable")])
        offset.append(offset[-1] + n)
    targets = np.concatenate(targets).astype(np.float32).reshape(-1, 6)
    if shuffle:
        targets = targets[rng.permutation(len(targets))]
    return np.concatenate(dets).astype(np.float32).reshape(-1, 6), offset, targets


# ------------------------------------------------------------------------------------------------------ the smallest cases
@pytest.mark.parametrize("case", ["hit", "miss", "wrong_class"])
def test_one_detection_one_label(case):
    box = {"hit": (100, 100, 200, 220), "miss": (300, 300, 400, 420), "wrong_class": (100, 100, 200, 220)}[case]
    cls = 1.0 if case == "wrong_class" else 2.0
    det = [[*box, 0.9, cls]]
    targets = [[0, 2, 150, 160, 100, 120]]
    predn, correct, cm = _check(det, [0, 1], targets, [GEOMS["unit"]], nc=3)
    assert correct.all() == (case == "hit") and correct.any() == (case == "hit")
    want = np.zeros((4, 4), int)
    if case == "miss":
        want[3, 2] = 1                                               # no claim at all: the detection adds nothing
    else:
        want[int(cls), 2] = 1
    np.testing.assert_array_equal(cm, want)


def test_batch_with_empty_images():
    """B = 4: an image without detections, one without labels, one with neither, one with both."""
    det, offset, targets = _scene(1, n_lab=[5, 0, 0, 4], n_det=[0, 6, 0, 7], nc=3)
    predn, correct, cm = _check(det, offset, targets, [GEOMS["unit"]] * 4, nc=3)
    assert not correct[:6].any()                                     # image 1 has no labels: its rows are zero ...
    assert cm[3, :3].sum() >= 5                                      # ... and image 0's labels are all background misses


def test_no_detection_in_the_whole_batch():
    _, offset, targets = _scene(2, n_lab=[3, 2], n_det=[0, 0], nc=2)
    predn, correct, cm = _check(np.zeros((0, 6)), offset, targets, [GEOMS["unit"]] * 2, nc=2)
    assert predn.shape == (0, 6) and correct.shape == (0, 10) and cm[2, :2].sum() == 5


def test_targets_in_shuffled_row_order():
    det, offset, targets = _scene(3, n_lab=[6, 9, 4], n_det=[8, 11, 5], nc=4, shuffle=True)
    assert (np.diff(targets[:, 0]) < 0).any()                        # the rows of an image are not contiguous
    _check(det, offset, targets, [GEOMS["pad_x"], GEOMS["unit"], GEOMS["pad_y"]], nc=4)


@pytest.mark.parametrize("nc,T", [(1, 10), (80, 1), (80, 10), (1, 1)])
def test_beyond_one_round_and_one_label_chunk(nc, T):
    """Image 0: THREADS + 44 detections (a second round of the workgroup) on 2 * CHUNK + 7 labels (three LDS chunks, the last
    partial), rows shuffled; image 1: more labels than detections; image 2: CHUNK labels exactly."""
    det, offset, targets = _scene(10 + nc + T, n_lab=[2 * CHUNK + 7, 40, CHUNK], n_det=[THREADS + 44, 5, 70], nc=nc, shuffle=True,
                                  spread=0.4)
    predn, correct, cm = _check(det, offset, targets, [GEOMS["pad_y"], GEOMS["unit"], GEOMS["pad_x"]], nc=nc, T=T)
    assert correct[:THREADS + 44].any() and correct[THREADS:THREADS + 44].shape[0] == 44
    credited = cm[:nc, :nc].sum()
    assert credited > 20 and cm[nc, :nc].sum() + credited == len(targets)      # every label is credited or missed, once


@pytest.mark.parametrize("geom", sorted(GEOMS))
def test_geometry_and_clip(geom):
    """Each letterbox geometry, with boxes that leave the image on every side (so that every clamp acts) and a zero-area
    detection."""
    det, offset, targets = _scene(20, n_lab=[7], n_det=[12], nc=3)
    det[0, :4] = (-20, -30, 600, 700)                                # beyond the frame on all four sides
    det[1, :4] = (-50, 100, 40, 200)
    det[2, :4] = (300, -60, 380, 30)
    det[3, :4] = (100, 100, 100, 100)                                # zero area
    det[4, :4] = (470, 480, 700, 800)
    targets[0, 2:] = (256, 256, 700, 800)                            # a label larger than the frame
    targets[1, 2:] = (5, 256, 80, 100)                               # and one over the left edge
    predn, correct, cm = _check(det, offset, targets, [GEOMS[geom]], nc=3)
    h0, w0 = GEOMS[geom][3:]
    assert predn[0, :4].tolist() == [0, 0, w0, h0]
    assert predn[3, 0] == predn[3, 2] and predn[3, 1] == predn[3, 3]


# ------------------------------------------------------------------------------------------------------ exact lattice cases
def test_iou_exactly_at_a_level_counts():
    """label [0,0,2,2] against detection [0,0,4,2]: IoU = 4 / (4 + 8 - 4 + 1e-7f) = 4 / 8 exactly (8 + 1e-7f == 8): a true
    positive at level 0.5 (>=) and not at 0.55."""
    predn, correct, cm = _check([[0, 0, 4, 2, 0.9, 0]], [0, 1], [[0, 0, 1, 1, 2, 2]], [GEOMS["unit"]], nc=1)
    assert correct[0].tolist() == [True] + [False] * 9
    np.testing.assert_array_equal(cm, [[1, 0], [0, 0]])              # 0.5 > 0.45: a confusion match


def test_iou_exactly_at_the_confusion_threshold_is_no_match():
    """label [0,0,4,5] against detection [0,0,3,3]: IoU = 9 / 20 = 0.45f exactly: no confusion match (strict >)."""
    predn, correct, cm = _check([[0, 0, 3, 3, 0.9, 0]], [0, 1], [[0, 0, 2, 2.5, 4, 5]], [GEOMS["unit"]], nc=1)
    assert not correct.any()
    np.testing.assert_array_equal(cm, [[0, 0], [1, 0]])


def test_ties():
    """Our definition: of equal IoUs the lowest label index, then the lowest detection index."""
    # two detections (mirror images: equal IoU) on one label
    det = [[8, 10, 28, 30, 0.9, 1], [12, 10, 32, 30, 0.8, 1], [12, 10, 32, 30, 0.7, 0]]
    predn, correct, cm = _check(det, [0, 3], [[0, 1, 20, 20, 20, 20]], [GEOMS["unit"]], nc=2)
    assert correct[0].any() and not correct[1:].any()
    np.testing.assert_array_equal(cm, [[0, 0, 1], [0, 1, 1], [0, 0, 0]])
    # one detection on two identical labels (of different classes for the confusion matrix to tell them apart)
    det = [[10, 10, 30, 30, 0.9, 1]]
    predn, correct, cm = _check(det, [0, 1], [[0, 0, 20, 20, 20, 20], [0, 1, 20, 20, 20, 20]], [GEOMS["unit"]], nc=2)
    assert correct[0].all()
    np.testing.assert_array_equal(cm, [[0, 0, 0], [1, 0, 0], [0, 1, 0]])     # it claims label 0 (class 0); label 1 is missed
    # ... and of the same class: one true positive, one credited label
    predn, correct, cm = _check(det, [0, 1], [[0, 1, 20, 20, 20, 20], [0, 1, 20, 20, 20, 20]], [GEOMS["unit"]], nc=2)
    assert correct[0].all()
    np.testing.assert_array_equal(cm, [[0, 0, 0], [0, 1, 0], [0, 1, 0]])


# ------------------------------------------------------------------------------------------------------ reference fixtures
def test_native_mode_reproduces_the_reference_correct_matrix(golden):
    """ADAYOLO_MATCH_NATIVE on evalharness.npz's det / lab: `correct` is the reference's process_batch result, predn is det."""
    g = golden("evalharness")
    det, lab = g["det"], g["lab"]
    targets = np.concatenate([np.zeros((len(lab), 1), np.float32), lab], 1)
    nc = int(max(det[:, 5].max(), lab[:, 0].max())) + 1
    predn, correct, cm = _check(det, [0, len(det)], targets, None, nc=nc, native=True)
    np.testing.assert_array_equal(correct.numpy(), g["correct"])
    assert np.array_equal(predn.numpy().view(np.uint32), det.view(np.uint32))


def test_packed_batch_reproduces_the_reference_confusion_matrix(golden):
    g = golden("confusion")
    nc = int(g["nc"])
    predn, correct, cm = _check(g["batch.det"], g["batch.offset"].tolist(), g["batch.targets"], None, nc=nc, native=True)
    np.testing.assert_array_equal(cm, g["total"])


def test_two_calls_accumulate_and_null_confusion_changes_nothing():
    det, offset, targets = _scene(30, n_lab=[6, 5], n_det=[9, 8], nc=3)
    geom = [GEOMS["pad_x"], GEOMS["unit"]]
    iouv = _iouv(10)
    buf = torch.zeros(16, dtype=torch.int32, device=DEV)
    predn1, correct1, cm1 = _run(det, offset, targets, geom, iouv, 3, confusion=buf)
    cm1 = cm1.copy()
    predn2, correct2, cm2 = _run(det, offset, targets, geom, iouv, 3, confusion=buf)
    assert cm1.sum() > 0
    np.testing.assert_array_equal(cm2, 2 * cm1)
    predn3, correct3, none = _run(det, offset, targets, geom, iouv, 3, confusion=None)
    assert none is None and torch.equal(correct3, correct1) and torch.equal(correct2, correct1) and torch.equal(predn3, predn1)
    assert (buf.cpu().numpy().reshape(4, 4) == cm2).all()            # the third call left the buffer alone


def test_confusion_matrix_object_reads_its_device_counts_back(golden):
    """ConfusionMatrix.process_batch_device: host and device counts add up in `.matrix`."""
    from adaptiveisp_amd.val import ConfusionMatrix
    g = golden("confusion")
    nc = int(g["nc"])
    cm = ConfusionMatrix(nc)
    cm.process_batch(torch.from_numpy(g["det5"]), torch.from_numpy(g["lab5"]))
    args = (torch.from_numpy(g["batch.det"]).to(DEV), torch.from_numpy(g["batch.offset"]).to(DEV),
            torch.from_numpy(g["batch.targets"]).to(DEV), None, _iouv(10))
    cm.process_batch_device(*args, native=True)
    np.testing.assert_array_equal(cm.matrix, g["total"] + g["cm5"])
    cm.process_batch_device(*args, native=True)
    np.testing.assert_array_equal(cm.matrix, 2 * g["total"] + g["cm5"])
    assert cm.matrix.dtype.kind == "i"


def test_host_path_on_the_device_is_within_one_ulp_of_the_kernel():
    """The contract between run_eval's two modes at a gain whose reciprocal is not exact (0.512). The host path ON A HIP DEVICE
    is not the host path on CPU tensors: torch divides a device tensor by a Python scalar as x * fl(1 / gain). The bound, by
    reasoning: with q the exact quotient in a binade of spacing u, fl(x / gain) is within u / 2 of q; x * fl(1 / gain) carries
    the reciprocal's relative error <= 2^-24, i.e. less than u, plus u / 2 of its own rounding: less than 3u / 2 from q. Two
    floats less than 2u apart are at most ONE spacing apart, and the clamp is monotone. So: native-space boxes of the two
    paths differ by at most one ulp — and where no IoU of the image lies within 1e-5 of a level or of the confusion threshold
    (a property of this seeded scene, asserted; a last-bit change of a box moves an IoU by ~1e-7), `correct` and the confusion
    matrix are equal."""
    from adaptiveisp_amd.val import ConfusionMatrix, box_iou, process_batch, scale_boxes, xywh2xyxy
    det, offset, targets = _scene(61, n_lab=[12], n_det=[30], nc=3)
    geom = GEOMS["pad_x"]
    iouv = _iouv(10)
    predn, correct, cm = _check(det, offset, targets, [geom], nc=3)                      # the kernel == the CPU host path
    gain, px, py, h0, w0 = geom
    ratio_pad = ((gain, gain), (px, py))
    pred_d, lab_d = torch.from_numpy(det).to(DEV), torch.from_numpy(targets[:, 1:]).to(DEV)
    predn_d = pred_d.clone()
    scale_boxes(NET, predn_d[:, :4], (h0, w0), ratio_pad)
    labelsn_d = torch.cat((lab_d[:, 0:1], scale_boxes(NET, xywh2xyxy(lab_d[:, 1:5]), (h0, w0), ratio_pad)), 1)
    a, b = predn_d.cpu().numpy(), predn.numpy()
    assert (np.abs(a - b) <= np.spacing(np.maximum(np.abs(a), np.abs(b)))).all()
    assert (a != b).any()                                            # the two divisions do differ at this gain
    iou = box_iou(labelsn_d[:, 1:], predn_d[:, :4]).cpu().numpy()
    edges = np.concatenate([iouv.cpu().numpy(), [np.float32(0.45)]])
    assert np.abs(iou[:, :, None] - edges[None, None, :]).min() > 1e-5
    assert torch.equal(process_batch(predn_d, labelsn_d, iouv).cpu(), correct)
    cm_d = ConfusionMatrix(3)
    cm_d.process_batch(predn_d, labelsn_d)
    np.testing.assert_array_equal(cm_d.matrix, cm)
    assert cm[:3, :3].sum() > 3 and correct.any()


# ------------------------------------------------------------------------------------------------------ the harness
NC_EVAL = 4


class _TableDetector:
    """A detector stand-in that a hipGraph can capture: fixed rows around the labels of its images (some with another class,
    some strays), every box shifted by a multiple of the retouched image's mean so that batches differ."""

    def __init__(self, B, H, W, seed):
        rng = np.random.default_rng(seed)
        n = 12
        self.labels = []
        table = np.zeros((B, 24, 5 + NC_EVAL), np.float32)
        for b in range(B):
            m = [3, 0, 5][b % 3]                                     # the second image of a batch has no labels
            lab = np.concatenate([rng.integers(0, NC_EVAL, (m, 1)), rng.uniform(0.3, 0.7, (m, 2)), rng.uniform(0.15, 0.4, (m, 2))], 1)
            self.labels.append(lab)
            for i in range(n if b != 2 else 0):                      # the third has labels and no detection
                if m and i < 8:
                    k = i % m
                    table[b, i, :4] = lab[k, 1:] * (W, H, W, H) + rng.normal(0, 1.5, 4)
                    c = int(lab[k, 0]) if i % 3 else int(rng.integers(0, NC_EVAL))
                else:
                    table[b, i, :4] = (*rng.uniform(10, 80, 2), *rng.uniform(8, 30, 2))
                    c = int(rng.integers(0, NC_EVAL))
                table[b, i, 4] = rng.uniform(0.3, 0.95)
                table[b, i, 5 + c] = rng.uniform(0.5, 0.95)
        self.table = torch.from_numpy(table).to(DEV)

    def __call__(self, x):
        shift = x.mean(dim=(1, 2, 3)) * 4.0
        out = self.table[:x.shape[0]].clone()
        out[:, :, :2] += shift[:, None, None]
        return out


@pytest.fixture(scope="module")
def eval_agent():
    from _synth import synth_state_dict
    from adaptiveisp_amd.agent import Agent
    from adaptiveisp_amd.config import cfg
    torch.manual_seed(0)
    agent = Agent(cfg, shape=(6 + len(cfg.filters), 64, 64), device=DEV).to(DEV)
    agent.load_state_dict(synth_state_dict(agent, seed=0))
    return agent.eval()


@pytest.mark.parametrize("graph", [False, True])
@pytest.mark.parametrize("single_cls", [False, True])
@pytest.mark.parametrize("B", [1, 3])
def test_run_eval_device_matching_equals_host_matching(eval_agent, B, single_cls, graph):
    """run_eval(match="device", confusion=True) against run_eval(match="host", confusion=True) on the same batches. The
    letterbox gains are 1 and 0.5 — with padding on x, on y, and from the `ratio_pad=None` arithmetic: the host path on a HIP
    device divides the boxes by a Python scalar, which torch does there as a multiplication by the reciprocal, so the two paths
    are the same arithmetic only where 1 / gain is exact (any other gain: one ulp apart at most,
    test_host_path_on_the_device_is_within_one_ulp_of_the_kernel)."""
    from adaptiveisp_amd.config import cfg
    from adaptiveisp_amd.val import run_eval
    H, W = 96, 128
    det = _TableDetector(B, H, W, seed=40 + B)
    shapes = [((H, W), ((1.0, 1.0), (0.0, 0.0))), ((192, 192), ((0.5, 0.5), (16.0, 0.0))), ((128, 256), ((0.5, 0.5), (0.0, 16.0))),
              ((192, 256), None)]
    g = torch.Generator().manual_seed(50)
    batches = []
    for i in range(3):
        t = np.concatenate([np.concatenate([np.full((len(det.labels[b]), 1), b), det.labels[b]], 1) for b in range(B)])
        t = torch.from_numpy(t.astype(np.float32))
        if single_cls:
            t[:, 1] = 0
        batches.append((torch.rand(B, 3, H, W, generator=g) * 0.6, t, [f"im{i}_{b}.png" for b in range(B)],
                        [shapes[(i + b) % 4] for b in range(B)]))
    nc = 1 if single_cls else NC_EVAL
    out = {}
    for mode in ("host", "device"):
        np.random.seed(3)
        details, images = [], []
        res = run_eval(eval_agent, det, batches, cfg, steps=2, conf_thres=0.2, nc=nc, single_cls=single_cls, graph=graph,
                       details=details, on_image=lambda p, predn, shape: images.append((p, predn.clone(), shape)),
                       match=mode, confusion=True)
        out[mode] = (res, details, images)
    (rh, dh, ih), (rd, dd, idv) = out["host"], out["device"]
    assert rh["seen"] == rd["seen"] == 3 * B and rh["records"] == rd["records"]
    for k in ("map", "map50", "mp", "mr"):
        assert rh[k] == rd[k], k
    assert np.array_equal(rh["ap"], rd["ap"]) and np.array_equal(rh["nt"], rd["nt"]) and np.array_equal(rh["ap_class"], rd["ap_class"])
    assert rh["map50"] > 0 and rh["nt"].sum() == 3 * sum(len(det.labels[b]) for b in range(B))
    assert len(dh) == len(dd) == 3 * B
    for a, b in zip(dh, dd):
        assert a["path"] == b["path"] and torch.equal(a["pred"], b["pred"])
        assert (a["correct"] is None) == (b["correct"] is None)
        if a["correct"] is not None:
            assert a["correct"].dtype == b["correct"].dtype == torch.bool and torch.equal(a["correct"], b["correct"])
    assert len(ih) == len(idv) > 0
    for (pa, na, sa), (pb, nb, sb) in zip(ih, idv):
        assert pa == pb and sa == sb and torch.equal(na, nb)
    np.testing.assert_array_equal(rh["confusion"], rd["confusion"])
    m = rd["confusion"]
    assert m.sum() > 0 and m[:nc, :nc].sum() + m[nc, :nc].sum() == rh["nt"].sum()       # every label credited or missed, once
    if B == 3:
        assert m[nc, :nc].sum() >= 3 * len(det.labels[2])            # the image without detections: background misses


def test_device_matching_on_a_cpu_device_is_an_error():
    from _engine import cpu_agent
    from adaptiveisp_amd.config import cfg
    from adaptiveisp_amd.val import run_eval
    with pytest.raises(ValueError, match="HIP device"):
        run_eval(cpu_agent(cfg), lambda x: x, [], cfg, match="device")


def test_cli_writes_the_confusion_csv(tmp_path):
    """python -m adaptiveisp_amd.val --match device --confusion --verbose: confusion_matrix.csv beside records.txt, every label
    of the set in exactly one cell of its column."""
    from PIL import Image
    from _synth import synth_state_dict
    from adaptiveisp_amd.agent import Agent
    from adaptiveisp_amd.config import cfg
    os.makedirs(tmp_path / "data" / "images"); os.makedirs(tmp_path / "data" / "labels")
    rng = np.random.default_rng(21)
    n_labels = 0
    for i, (h, w) in enumerate([(150, 200), (128, 96), (120, 120)]):
        im = np.kron(rng.random((h // 8 + 1, w // 8 + 1, 3)), np.ones((8, 8, 1)))[:h, :w] * 0.4 + rng.random((h, w, 3)) * 0.1
        Image.fromarray((im * 255).astype(np.uint8)).save(tmp_path / "data" / "images" / f"img{i}.png")
        lb = np.concatenate([rng.integers(0, 7, (2 + i, 1)).astype(np.float64), rng.uniform(0.25, 0.75, (2 + i, 2)),
                             rng.uniform(0.1, 0.4, (2 + i, 2))], 1)
        np.savetxt(tmp_path / "data" / "labels" / f"img{i}.txt", lb, fmt="%.6f")
        n_labels += len(lb)
    agent = Agent(cfg, shape=(6 + len(cfg.filters), 64, 64))
    torch.save({"iter": 0, "agent_model": synth_state_dict(agent, seed=0)}, tmp_path / "agent.pth")
    cmd = ["timeout", "-k", "10", "300", sys.executable, "-m", "adaptiveisp_amd.val", "--isp-ckpt", str(tmp_path / "agent.pth"),
           "--detector-ckpt", os.path.join(GOLD, "yolov3_w0625_refpickle.pt"), "--data", str(tmp_path / "data" / "images"),
           "--img-size", "128", "--batch-size", "2", "--project", str(tmp_path / "runs"), "--match", "device", "--confusion",
           "--verbose", "--graph"]
    env = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
    r = subprocess.run(cmd, cwd=ROOT, env=env, capture_output=True, text=True)
    assert r.returncode == 0, f"exit {r.returncode}\n{r.stdout[-3000:]}\n{r.stderr[-3000:]}"
    run = tmp_path / "runs" / "exp"
    assert (run / "records.txt").exists() and "Missed" in r.stdout
    rows = [line.split(",") for line in (run / "confusion_matrix.csv").read_text().strip().split("\n")]
    assert rows[0][-1] == "background" and len(rows) == len(rows[0]) == 7 + 2
    m = np.array([[int(v) for v in row[1:]] for row in rows[1:]])
    assert m[:, :7].sum() == n_labels
    # ... and the counts are those of run_eval on the same data, rows and columns under the detector's class names
    from adaptiveisp_amd.val import run_eval
    from adaptiveisp_amd.val.loader import LODImages
    from adaptiveisp_amd.yolo import YoloEngine
    from adaptiveisp_amd.yolo.checkpoint import load_detector_checkpoint
    det = load_detector_checkpoint(os.path.join(GOLD, "yolov3_w0625_refpickle.pt")).to(DEV).eval()
    names = det.names if isinstance(det.names, dict) else dict(enumerate(det.names))
    assert rows[0][1:-1] == [str(names[c]) for c in range(7)] and [r[0] for r in rows[1:]] == rows[0][1:]
    agent = Agent(cfg, shape=(6 + len(cfg.filters), 64, 64), device=DEV).to(DEV)
    agent.load_state_dict(synth_state_dict(agent, seed=0))
    agent.eval()
    engines = {b: YoloEngine(det, b, 128, 128, device=DEV) for b in (2, 1)}
    np.random.seed(0)
    res = run_eval(agent, lambda x: engines[x.shape[0]](x), list(LODImages(str(tmp_path / "data" / "images"), img_size=128, batch_size=2)),
                   cfg, steps=5, nc=7, match="device", confusion=True)
    np.testing.assert_array_equal(m, res["confusion"])
