"""The confusion matrix of the evaluation on the host (no GPU): val.ConfusionMatrix against the matrices the REFERENCE's
ConfusionMatrix.process_batch fills (tests/golden/confusion.npz, written by tests/golden/gen_confusion.py), the tie
definition, run_eval(confusion=True) on the CPU, the CSV the CLI writes, and the argument checks of adayolo_match."""
import ctypes
import os
import subprocess

import numpy as np
import pytest
import torch

from adaptiveisp_amd.val import ConfusionMatrix
from adaptiveisp_amd.val import __main__ as cli
from adaptiveisp_amd.val import writers

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _feed(cm, det, lab):
    """One image as the evaluation loop hands it over: no detections at all -> detections=None."""
    cm.process_batch(torch.from_numpy(det) if len(det) else None, torch.from_numpy(lab))


def test_reproduces_the_reference_matrices(golden):
    g = golden("confusion")
    nc, n = int(g["nc"]), int(g["n_images"])
    assert n >= 36 and g["batch.offset"].shape == (n + 1,)
    total = ConfusionMatrix(nc)
    seen = dict(no_labels=0, no_dets=0, low_conf=0, both=0)
    for i in range(n):
        det, lab = g[f"det{i}"], g[f"lab{i}"]
        one = ConfusionMatrix(nc)
        _feed(one, det, lab)
        _feed(total, det, lab)
        assert one.matrix.dtype.kind == "i" and one.matrix.shape == (nc + 1, nc + 1)
        np.testing.assert_array_equal(one.matrix, g[f"cm{i}"], err_msg=f"image {i}")
        seen["no_labels"] += len(lab) == 0 and len(det) > 0
        seen["no_dets"] += len(det) == 0 and len(lab) > 0
        seen["low_conf"] += len(det) > 0 and len(lab) > 0 and bool((det[:, 4] <= 0.25).all())
        seen["both"] += len(det) > 0 and len(lab) > 0
    assert all(seen.values()), seen                                  # the fixture holds every empty case
    np.testing.assert_array_equal(total.matrix, g["total"])
    assert total.matrix.sum() == g["total"].sum() > 300
    # the packed batch is the same data
    off = g["batch.offset"]
    for i in (0, 7, n - 1):
        np.testing.assert_array_equal(g["batch.det"][off[i]:off[i + 1]], g[f"det{i}"])
        rows = g["batch.targets"][g["batch.targets"][:, 0] == i]
        np.testing.assert_array_equal(rows[:, 1:], g[f"lab{i}"])


def test_ties_go_to_the_lowest_label_then_the_lowest_detection():
    """Our definition (the reference leaves ties to an unstable sort): of equal IoUs the lowest label index, then the lowest
    detection index."""
    # two detections of different classes on one label with the same IoU (mirror images): detection 0 is credited
    lab = torch.tensor([[2.0, 10, 10, 30, 30]])
    det = torch.tensor([[8, 10, 28, 30, 0.9, 0.0], [12, 10, 32, 30, 0.8, 1.0]])
    cm = ConfusionMatrix(3)
    cm.process_batch(det, lab)
    want = np.zeros((4, 4), int)
    want[0, 2] = 1                                                   # detection 0 (class 0) on the class-2 label
    want[1, 3] = 1                                                   # detection 1: a background prediction
    np.testing.assert_array_equal(cm.matrix, want)
    cm = ConfusionMatrix(3)
    cm.process_batch(det.flip(0), lab)                               # the other order: now the class-1 detection is first
    want = np.zeros((4, 4), int)
    want[1, 2] = want[0, 3] = 1
    np.testing.assert_array_equal(cm.matrix, want)
    # one detection on two identical labels of different classes: it claims label 0; label 1 is missed
    lab = torch.tensor([[1.0, 10, 10, 30, 30], [2.0, 10, 10, 30, 30]])
    det = torch.tensor([[10, 10, 30, 30, 0.9, 0.0]])
    cm = ConfusionMatrix(3)
    cm.process_batch(det, lab)
    want = np.zeros((4, 4), int)
    want[0, 1] = want[3, 2] = 1
    np.testing.assert_array_equal(cm.matrix, want)


def test_threshold_is_strict_and_no_claim_means_no_background_predictions():
    lab = torch.tensor([[0.0, 0, 0, 4, 5]])
    det = torch.tensor([[0, 0, 3, 3, 0.9, 0.0]])                     # IoU 9 / 20 == 0.45f exactly: no match (strict >)
    cm = ConfusionMatrix(2)
    cm.process_batch(det, lab)
    want = np.zeros((3, 3), int)
    want[2, 0] = 1                                                   # the label is missed; the detection adds nothing
    np.testing.assert_array_equal(cm.matrix, want)
    cm = ConfusionMatrix(2, iou_thres=0.44)
    cm.process_batch(det, lab)
    want = np.zeros((3, 3), int)
    want[0, 0] = 1
    np.testing.assert_array_equal(cm.matrix, want)


def test_none_detections_are_background_misses():
    cm = ConfusionMatrix(4)
    cm.process_batch(None, torch.tensor([1.0, 3.0, 3.0]))            # label classes, as val_adaptiveisp.py:357 passes them
    cm.process_batch(None, torch.tensor([[0.0, 1, 1, 5, 5]]))        # or label rows
    want = np.zeros((5, 5), int)
    want[4, 1], want[4, 3], want[4, 0] = 1, 2, 1
    np.testing.assert_array_equal(cm.matrix, want)


def test_tp_fp_and_normalized():
    cm = ConfusionMatrix(3)
    cm._host[:] = np.array([[5, 1, 0, 2],
                            [0, 3, 1, 0],
                            [1, 0, 0, 4],
                            [2, 1, 0, 0]])
    tp, fp = cm.tp_fp()
    assert tp.tolist() == [5, 3, 0] and fp.tolist() == [3, 1, 5]
    norm = cm.normalized()
    np.testing.assert_allclose(norm.sum(0), [1, 1, 1, 1], atol=1e-8)
    np.testing.assert_allclose(norm[:, 0], np.array([5, 0, 1, 2]) / (8 + 1e-9), rtol=0, atol=1e-15)
    np.testing.assert_array_equal(ConfusionMatrix(2).normalized(), np.zeros((3, 3)))     # an empty column stays 0


def _oracle_nms_fn(oracle_mod):
    def fn(boxes, scores, thr):
        order = torch.argsort(scores, descending=True, stable=True)
        keep = oracle_mod.nms(boxes[order].numpy(), thr, max_det=max(boxes.shape[0], 1))
        return order[torch.from_numpy(keep)]
    return fn


def _cpu_eval(oracle_mod, **kw):
    from _engine import cpu_agent
    from adaptiveisp_amd.config import cfg
    from adaptiveisp_amd.val import run_eval
    agent = cpu_agent(cfg)
    g = torch.Generator().manual_seed(3)
    imgs = torch.rand(3, 3, 64, 96, generator=g) * 0.5
    targets = torch.tensor([[0, 1, 0.30, 0.40, 0.20, 0.30], [0, 2, 0.70, 0.55, 0.25, 0.30], [1, 0, 0.52, 0.48, 0.30, 0.35],
                            [2, 2, 0.40, 0.40, 0.20, 0.20]])

    def detector(x):
        pred = torch.zeros(3, 8, 5 + 3)
        for k, t in enumerate(targets[:3]):
            b, c = int(t[0]), int(t[1])
            row = int((pred[b, :, 4] > 0).sum())
            pred[b, row, :4] = t[2:] * torch.tensor([96., 64., 96., 64.])
            pred[b, row, 4] = 0.9
            pred[b, row, 5 + (c if k else 0)] = 0.95                # the first label is detected as class 0: a confusion
        pred[0, 5, :4] = torch.tensor([10., 10., 8., 8.]); pred[0, 5, 4] = 0.5; pred[0, 5, 5] = 0.9   # a false positive
        return pred                                                  # image 2: a label, no detection

    details = []
    res = run_eval(agent, detector, [(imgs, targets, ["a.png", "b.png", "c.png"], [((64, 96), ((1.0, 1.0), (0.0, 0.0)))] * 3)],
                   cfg, steps=2, conf_thres=0.001, iou_thres=0.6, nc=3, nms_fn=_oracle_nms_fn(oracle_mod), details=details, **kw)
    return res, details, targets


def test_run_eval_fills_the_matrix_per_image(oracle_mod):
    from adaptiveisp_amd.val import scale_boxes, xywh2xyxy
    plain, _, _ = _cpu_eval(oracle_mod)
    assert "confusion" not in plain                                  # the default result is unchanged
    res, details, targets = _cpu_eval(oracle_mod, confusion=True)
    for k in ("map", "map50", "mp", "mr"):
        assert res[k] == plain[k]
    want = ConfusionMatrix(3)
    px = targets.clone()
    px[:, 2:] *= torch.tensor([96., 64., 96., 64.])
    for si, d in enumerate(details):
        lab = px[px[:, 0] == si, 1:]
        labn = torch.cat((lab[:, 0:1], scale_boxes((64, 96), xywh2xyxy(lab[:, 1:5]), (64, 96), ((1.0, 1.0), (0.0, 0.0)))), 1)
        if d["pred"].shape[0] == 0:
            want.process_batch(None, labn)
        else:
            predn = d["pred"].clone()
            scale_boxes((64, 96), predn[:, :4], (64, 96), ((1.0, 1.0), (0.0, 0.0)))
            want.process_batch(predn, labn)
    np.testing.assert_array_equal(res["confusion"], want.matrix)
    m = res["confusion"]
    assert m.dtype.kind == "i" and m.shape == (4, 4)
    assert m[0, 1] == 1 and m[2, 2] == 1 and m[0, 0] == 1            # the confusion, and the two right ones
    assert m[0, 3] == 1                                              # the false positive
    assert m[3, 2] == 1 and m.sum() == 5                             # image 2's label: a background miss
    # an instance handed in is added to
    mine = ConfusionMatrix(3)
    res2, _, _ = _cpu_eval(oracle_mod, confusion=mine)
    res3, _, _ = _cpu_eval(oracle_mod, confusion=mine)
    np.testing.assert_array_equal(res3["confusion"], 2 * m)
    np.testing.assert_array_equal(res2["confusion"], m)              # a result handed out earlier is not changed by later counts
    assert mine.matrix.sum() == 10 and mine.matrix is not mine.matrix


def test_device_matching_needs_a_hip_device(oracle_mod):
    with pytest.raises(ValueError, match="HIP device"):
        _cpu_eval(oracle_mod, match="device")
    with pytest.raises(ValueError, match="match="):
        _cpu_eval(oracle_mod, match="gpu")
    from adaptiveisp_amd.val import match_batch
    from adaptiveisp_amd.yolo._lib import AdayoloError
    with pytest.raises(AdayoloError, match="no CPU path"):
        match_batch(torch.zeros(1, 6), torch.zeros(2, dtype=torch.int32), torch.zeros(1, 6), torch.zeros(1, 5),
                    torch.linspace(0.5, 0.95, 10), 3)


def test_cli_options_and_the_csv_it_writes(oracle_mod, tmp_path):
    """`--match` / `--confusion` parse (default host / off), and the writer the CLI hands res["confusion"] to leaves a CSV whose
    counts are that matrix (the CLI itself needs the GPU: tests/test_gpu_match.py runs it)."""
    base = ["--isp-ckpt", "agent.pth", "--data", "images"]
    a = cli.parse_args(base)
    assert a.match == "host" and a.confusion is False
    a = cli.parse_args(base + ["--match", "device", "--confusion"])
    assert a.match == "device" and a.confusion is True
    with pytest.raises(SystemExit):
        cli.parse_args(base + ["--match", "cpu"])
    res, _, _ = _cpu_eval(oracle_mod, confusion=True)
    f = tmp_path / "confusion_matrix.csv"
    writers.save_confusion_csv(res["confusion"], {0: "person", 1: "bicycle, old", 2: "car"}, str(f))
    rows = [line.split(",") for line in f.read_text().strip().split("\n")]
    assert rows[0][1:] == ["person", "bicycle  old", "car", "background"]
    assert [r[0] for r in rows[1:]] == rows[0][1:]
    got = np.array([[int(v) for v in r[1:]] for r in rows[1:]])
    np.testing.assert_array_equal(got, res["confusion"])
    assert all(v.isdigit() for r in rows[1:] for v in r[1:])         # integer counts
    writers.save_confusion_csv(res["confusion"], ["a", "b"], str(f))         # a sequence of names, one missing
    assert f.read_text().split("\n")[0].split(",")[1:] == ["a", "b", "2", "background"]


def test_adayolo_match_argument_checks_without_gpu():
    """Refused before any launch: null pointers (ADAYOLO_EINVAL), n_iou outside 1..16, nc < 1, negative counts (-2); the
    ctypes mirror has the header's layout."""
    from adaptiveisp_amd.yolo import _lib
    L = _lib.load()
    assert "adayolo_match" in _lib.EXPORTS and _lib.ABI_VERSION == 10 and L.adayolo_abi_version() == 10
    assert ctypes.sizeof(_lib.MatchArgs) == 96
    fn = L.adayolo_match
    assert fn(None, None) == -1
    p = 0x10000000                                                   # a fake device address: every call fails its checks first

    def args(**over):
        a = _lib.MatchArgs()
        for k, v in dict(dict(det=p, det_offset=p, targets=p, n_targets=4, batch=2, geom=p, iouv=p, n_iou=10, nc=80, flags=0,
                              cm_conf=0.25, cm_iou=0.45, predn=p, correct=p, confusion=None), **over).items():
            setattr(a, k, v)
        return ctypes.byref(a)
    for name in ("det", "det_offset", "iouv", "predn", "correct", "targets", "geom"):
        assert fn(args(**{name: None}), None) == -1, name
    for over in (dict(n_iou=0), dict(n_iou=17), dict(n_iou=-1), dict(nc=0), dict(n_targets=-1), dict(batch=-1), dict(flags=2)):
        assert fn(args(**over), None) == -2, over
    assert fn(args(n_iou=0, det=None), None) == -1                   # a null pointer is reported first
    assert fn(args(batch=0), None) == 0                              # nothing to do: no launch
    assert fn(args(batch=0, geom=None, flags=_lib.MATCH_NATIVE, targets=None, n_targets=0), None) == 0


def test_regen_check_confusion_reproduces_the_fixture():
    """tools/regen_check.sh confusion: the generator, run against the reference, rewrites confusion.npz with 0 differences
    (where the reference checkout is present: the build container)."""
    import re
    # where the generator looks for the reference, read from its text: importing it (matplotlib, gen_golden's environment) is
    # the generator's business and happens in the subprocess below, where a failure is a failure
    text = open(os.path.join(ROOT, "tests", "golden", "gen_confusion.py")).read()
    ref = re.search(r'def import_reference_metrics\(root="([^"]+)"\)', text).group(1)
    if not os.path.isdir(ref):
        pytest.skip("the reference checkout is not on this machine")
    r = subprocess.run(["bash", os.path.join(ROOT, "tools", "regen_check.sh"), "confusion"], cwd=ROOT, capture_output=True,
                       text=True, timeout=600)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "confusion.npz: 129 arrays, 0 differing" in r.stdout and "0 differences" in r.stdout
