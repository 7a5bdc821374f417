"""adayolo_nms_batch (csrc/yolo_nms_batch.hip) against the host path: `val.non_max_suppression` on CPU fp32 tensors with the C
oracle's greedy NMS injected — the combination tests/golden/evalharness.npz pins to the reference. The device result has to be
EQUAL: the same number of rows per image, in the same order, torch.equal on all six columns. No tolerance anywhere.

Sizes are the smallest at which the kernels take another path: the NMS works in blocks of 64 candidates, the sort in LDS tiles
of 4096 keys (more keys: passes over global memory), 1024 threads per image."""
import json
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


def _oracle(oracle_mod):
    def fn(boxes, scores, thr):
        order = torch.argsort(scores, descending=True, stable=True)
        keep = oracle_mod.nms(boxes[order].numpy(), thr, max_det=max(boxes.shape[0], 1))
        return order[torch.from_numpy(keep)]
    return fn


def _yard(oracle_mod, pred, conf, iou, multi, agn, max_det):
    from adaptiveisp_amd.val import non_max_suppression
    return non_max_suppression(pred.detach().cpu().clone(), conf, iou, multi_label=multi, agnostic=agn, max_det=max_det,
                               nms_fn=_oracle(oracle_mod))


def _device(pred, conf, iou, multi, agn, max_det, max_nms=30000, cap=None, **kw):
    from adaptiveisp_amd.yolo import _lib
    if cap is None:
        cap = max(1, pred.shape[1] * (pred.shape[2] - 5))
    det, off, status = _lib.nms_batch(pred, conf, iou, max_det, max_nms, cap, multi, agn, **kw)
    torch.cuda.synchronize()
    off = off.cpu().tolist()
    assert off[0] == 0 and len(off) == pred.shape[0] + 1 and det.shape == (max(pred.shape[0] * max_det, 1), 6)
    return [det[off[b]:off[b + 1]].cpu() for b in range(pred.shape[0])], status.cpu().tolist()


def _same(got, ref, images=None):
    assert len(got) == len(ref)
    for b in (range(len(ref)) if images is None else images):
        assert got[b].shape == ref[b].shape, (b, got[b].shape, ref[b].shape)
        assert torch.equal(got[b], ref[b]), (b, (got[b] != ref[b]).nonzero()[:5])


def _check(oracle_mod, pred, conf=0.25, iou=0.45, multi=False, agn=False, max_det=300):
    ref = _yard(oracle_mod, pred, conf, iou, multi, agn, max_det)
    got, status = _device(pred.to(DEV), conf, iou, multi, agn, max_det)
    assert status == [0] * pred.shape[0]
    _same(got, ref)
    return ref


def _clustered(rng, B, N, nc, centres=6, size=(20.0, 60.0), jitter=6.0):
    """Rows around a handful of cluster centres per image, so that boxes overlap and suppression really happens."""
    pred = np.zeros((B, N, 5 + nc), np.float32)
    for b in range(B):
        c = rng.uniform(80, 560, (centres, 2))
        s = rng.uniform(*size, (centres, 2))
        k = rng.integers(0, centres, N)
        pred[b, :, :2] = c[k] + rng.normal(0, jitter, (N, 2))
        pred[b, :, 2:4] = s[k] * rng.uniform(0.8, 1.25, (N, 2))
        pred[b, :, 4] = rng.uniform(0, 1, N)
        pred[b, :, 5:] = rng.uniform(0, 1, (N, nc))
    return torch.from_numpy(pred)


@pytest.mark.parametrize("tag", ["ml", "best", "agn"])
def test_golden(golden, oracle_mod, tag):
    """The reference's own results (tests/golden/gen_golden.py::gen_eval) for the stored prediction and keyword arguments."""
    from test_eval_harness import CASES
    g, kw = golden("evalharness"), CASES[tag]
    pred = torch.from_numpy(g["pred"].copy())
    got, status = _device(pred.to(DEV), kw["conf_thres"], kw["iou_thres"], kw["multi_label"], kw.get("agnostic", False), kw["max_det"])
    assert status == [0, 0]
    for b in range(2):
        ref = torch.from_numpy(g[f"nms.{tag}.{b}"])
        assert got[b].shape == ref.shape and torch.equal(got[b], ref)   # bit-exact, as the host path is held to it
    _same(got, _yard(oracle_mod, pred, kw["conf_thres"], kw["iou_thres"], kw["multi_label"], kw.get("agnostic", False), kw["max_det"]))


def _segments(rng, counts, nc=1):
    """Images with exactly counts[b] candidates (best-class mode, conf 0.25), the other rows below the threshold."""
    N = max(max(counts), 1) + 9
    pred = _clustered(rng, len(counts), N, nc)
    for b, k in enumerate(counts):
        on = rng.permutation(N)[:k]
        pred[b, :, 4] = 0.1
        pred[b, on, 4] = torch.from_numpy(rng.uniform(0.6, 1.0, k).astype(np.float32))
        pred[b, :, 5:] = torch.from_numpy(rng.uniform(0.6, 1.0, (N, nc)).astype(np.float32))
    return pred


@pytest.mark.parametrize("counts", [[0, 1, 64 * 2 + 7], [64 * 2 + 7], [0], [1], [64], [65], [0, 0]])
def test_segment_shapes(oracle_mod, counts):
    """No candidate, exactly one, and two full NMS blocks plus a partial one, in one batch and alone."""
    rng = np.random.default_rng(100 + len(counts) + counts[-1])
    pred = _segments(rng, counts)
    ref = _check(oracle_mod, pred, iou=0.45)
    open_ = _yard(oracle_mod, pred, 0.25, 1.0, False, False, 10 ** 6)
    assert [r.shape[0] for r in open_] == counts                      # the case is the one its name says
    if counts[-1] > 64:
        assert 1 < ref[-1].shape[0] < counts[-1]                      # suppression happened and something survived


def test_ties_have_one_order(oracle_mod):
    """Equal scores across rows and across the classes of one row: the order is candidate order (row, then class), whatever
    order the atomic appends were served in — twice the same, and the host path's."""
    rng = np.random.default_rng(7)
    N, nc = 300, 3
    pred = _clustered(rng, 2, N, nc, centres=40, size=(8.0, 20.0))
    pred[:, :, 4] = torch.from_numpy(rng.choice(np.array([0.5, 0.75, 1.0], np.float32), (2, N)))
    pred[:, :, 5:] = torch.from_numpy(rng.choice(np.array([0.5, 1.0], np.float32), (2, N, nc)))
    pred[0, 10:20, 5:] = 0.5                                            # all classes of a row equal
    for multi in (True, False):
        ref = _check(oracle_mod, pred, conf=0.2, iou=0.5, multi=multi)
        assert all(len(torch.unique(r[:, 4])) < r.shape[0] / 4 for r in ref)          # ties among the kept rows
        a, _ = _device(pred.to(DEV), 0.2, 0.5, multi, False, 300)
        b, _ = _device(pred.to(DEV), 0.2, 0.5, multi, False, 300)
        _same(a, b)


def test_truncation_at_max_det(oracle_mod):
    rng = np.random.default_rng(8)
    pred = _clustered(rng, 2, 200, 2, centres=30, size=(8.0, 16.0))
    free = _yard(oracle_mod, pred, 0.25, 0.45, True, False, 300)
    assert all(r.shape[0] > 5 for r in free)
    ref = _check(oracle_mod, pred, multi=True, max_det=5)
    assert all(r.shape[0] == 5 for r in ref)
    _check(oracle_mod, pred, multi=True, max_det=1)
    _check(oracle_mod, pred, multi=True, max_det=64)
    _check(oracle_mod, pred, multi=True, max_det=2048)


def test_truncation_at_max_nms(oracle_mod, monkeypatch):
    """150 candidates, max_nms = 100: the host path cuts its sorted list at MAX_NMS, patched to 100 for this test only. The
    boxes are far apart, so everything that enters the NMS survives it: 100 rows, not 150."""
    from adaptiveisp_amd.val import nms
    rng = np.random.default_rng(9)
    pred = torch.zeros(2, 170, 6)
    pred[:, :, 0] = torch.arange(170) * 30.0
    pred[:, :, 1] = 50.0
    pred[:, :, 2:4] = 10.0
    pred[:, :, 4] = 0.1
    for b, k in enumerate((150, 99)):
        pred[b, torch.from_numpy(rng.permutation(170)[:k]), 4] = torch.from_numpy(rng.uniform(0.5, 1, k).astype(np.float32))
    pred[:, :, 5] = 1.0
    monkeypatch.setattr(nms, "MAX_NMS", 100)
    ref = _yard(oracle_mod, pred, 0.25, 0.45, False, False, 300)
    assert [r.shape[0] for r in ref] == [100, 99]
    got, status = _device(pred.to(DEV), 0.25, 0.45, False, False, 300, max_nms=100)
    assert status == [0, 0]
    _same(got, ref)


def _overflow_pred(rng):
    pred = _segments(rng, [40, 100, 64])
    return pred


def test_overflow_sets_the_status_and_spares_the_others(oracle_mod):
    rng = np.random.default_rng(10)
    pred = _overflow_pred(rng)
    ref = _yard(oracle_mod, pred, 0.25, 0.45, False, False, 300)
    got, status = _device(pred.to(DEV), 0.25, 0.45, False, False, 300, cap=64)
    assert status == [0, 1, 0]                                        # ADAYOLO_NMS_OVERFLOW; exactly cap candidates is no overflow
    _same(got, ref, images=(0, 2))
    assert got[1].shape[0] == 0                                       # the overflowed image gets no rows (include/adayolo.h)


class _FixedDetector:
    def __init__(self, table):
        self.table = table.to(DEV)

    def __call__(self, x):
        return self.table[:x.shape[0]].clone() + 0.0 * x.mean()


@pytest.fixture(scope="module")
def eval_agent():
    from _synth import synth_state_dict
    from adaptiveisp_amd.agent import Agent
    from adaptiveisp_amd.config import cfg
    torch.manual_seed(0)
    agent = Agent(cfg, shape=(6 + len(cfg.filters), 64, 64), device=DEV).to(DEV)
    agent.load_state_dict(synth_state_dict(agent, seed=0))
    return agent.eval()


def _labels(rng, B, nc, per_image):
    rows = []
    for b in range(B):
        m = per_image[b % len(per_image)]
        rows.append(np.concatenate([np.full((m, 1), b), rng.integers(0, nc, (m, 1)), rng.uniform(0.3, 0.7, (m, 2)),
                                    rng.uniform(0.15, 0.4, (m, 2))], 1))
    return torch.from_numpy(np.concatenate(rows).astype(np.float32))


def _equal_results(ra, da, rb, db):
    assert ra["seen"] == rb["seen"] and ra["records"] == rb["records"]
    for k in ("map", "map50", "mp", "mr"):
        assert ra[k] == rb[k], k
    for k in ("nt", "ap", "ap_class", "confusion"):
        assert np.array_equal(ra[k], rb[k]), k
    assert len(da) == len(db)
    for a, b in zip(da, db):
        assert a["path"] == b["path"] and torch.equal(a["pred"], b["pred"])
        assert (a["correct"] is None) == (b["correct"] is None)
        if a["correct"] is not None:
            assert torch.equal(a["correct"], b["correct"])


def test_run_eval_falls_back_on_overflow(eval_agent, monkeypatch):
    """cap = 64 (injected: run_eval itself uses the default) with 100 candidates in one image of three: that batch goes through
    the host function, the result says so, and nothing else differs from the host mode's."""
    from adaptiveisp_amd.config import cfg
    from adaptiveisp_amd.val import harness, run_eval
    rng = np.random.default_rng(10)
    pred = _overflow_pred(rng)
    pred[:, :, :4] *= 0.2                                             # inside the 128 x 128 image
    det = _FixedDetector(pred)
    targets = _labels(rng, 3, 1, [2, 3, 1])
    batches = [(torch.rand(3, 3, 128, 128) * 0.5, targets, [f"a{b}.png" for b in range(3)], [((128, 128), ((1.0, 1.0), (0.0, 0.0)))] * 3)]
    real = harness.non_max_suppression_device
    monkeypatch.setattr(harness, "non_max_suppression_device", lambda *a, **k: real(*a, **dict(k, cap=64)))
    out = {}
    for mode in ("host", "device"):
        np.random.seed(3)
        details = []
        out[mode] = (run_eval(eval_agent, det, batches, cfg, steps=2, conf_thres=0.25, iou_thres=0.45, nc=1, match="device",
                              nms=mode, details=details, confusion=True), details)
    assert out["device"][0]["nms_fallbacks"] == 1 and out["host"][0]["nms_fallbacks"] == 0
    _equal_results(*out["host"], *out["device"])
    assert sum(d["pred"].shape[0] for d in out["device"][1]) > 3


@pytest.mark.parametrize("agn", [False, True])
@pytest.mark.parametrize("multi", [False, True])
def test_flags(oracle_mod, multi, agn):
    rng = np.random.default_rng(11)
    pred = _clustered(rng, 2, 150, 3)
    ref = _check(oracle_mod, pred, conf=0.2, iou=0.5, multi=multi, agn=agn)
    assert all(1 < r.shape[0] for r in ref)


def test_one_class_takes_the_best_class_path_and_best_class_ties(oracle_mod):
    rng = np.random.default_rng(12)
    pred = _clustered(rng, 2, 150, 1)
    _check(oracle_mod, pred, conf=0.2, iou=0.5, multi=True)
    _check(oracle_mod, pred, conf=0.2, iou=0.5, multi=False)
    # two classes with the same product: the lowest index wins, as torch's max(dim) documents
    pred = torch.zeros(1, 4, 8)
    pred[0, :, 0] = torch.arange(4) * 100.0 + 50
    pred[0, :, 1:4] = torch.tensor([50.0, 20.0, 20.0])
    pred[0, :, 4] = 0.5
    pred[0, 0, 5:] = torch.tensor([0.25, 0.75, 0.75])
    pred[0, 1, 5:] = torch.tensor([0.75, 0.75, 0.25])
    pred[0, 2, 5:] = torch.tensor([0.75, 0.25, 0.75])
    pred[0, 3, 5:] = torch.tensor([0.5, 0.5, 0.5])
    ref = _check(oracle_mod, pred, conf=0.2, iou=0.5, multi=False)
    assert sorted(ref[0][:, 5].tolist()) == [0.0, 0.0, 0.0, 1.0]


@pytest.mark.parametrize("conf", [0.001, 0.25, 0.1])
def test_confidence_threshold_edges(oracle_mod, conf):
    """Objectness and products at float32(conf) and one ulp either side: `>` in fp32 (tests/test_nms_batch_host.py pins the
    host side of this)."""
    c32 = np.float32(conf)
    vals = [np.nextafter(c32, np.float32(-1)), c32, np.nextafter(c32, np.float32(2))]
    pred = torch.zeros(1, 12, 7)
    pred[0, :, 0] = torch.arange(12) * 40.0 + 20
    pred[0, :, 1:4] = torch.tensor([20.0, 10.0, 10.0])
    for i, v in enumerate(vals):
        pred[0, i, 4], pred[0, i, 5] = float(v), 1.0                     # at the objectness (the product is the same float)
        pred[0, 3 + i, 4], pred[0, 3 + i, 6] = 1.0, float(v)             # at the product alone
        pred[0, 6 + i, 4], pred[0, 6 + i, 5], pred[0, 6 + i, 6] = float(v), 1.0, 0.5   # objectness passes or not, one class below
        pred[0, 9 + i, 4], pred[0, 9 + i, 5], pred[0, 9 + i, 6] = 1.0, float(v), float(v)
    for multi in (False, True):
        ref = _check(oracle_mod, pred, conf=conf, iou=0.5, multi=multi)
        assert ref[0].shape[0] == (5 if multi else 4)


def _xywh(x1, y1, x2, y2):
    return [(x1 + x2) / 2, (y1 + y2) / 2, x2 - x1, y2 - y1]


@pytest.mark.parametrize("thr,at,above", [(0.5, (10, 5), (10, 6)), (0.6, (10, 6), (20, 13)), (0.25, (10, 5), (10, 6))])
def test_iou_threshold_edges_on_integer_lattices(oracle_mod, thr, at, above):
    """Box pairs whose IoU is exactly float32(thr) (kept: the rule is `>`) and just above it (suppressed). All coordinates are
    small integers or halves, so every fp32 operation before the division is exact, with and without the class offset."""
    rows = []
    big = {0.5: (10, 10), 0.6: (10, 10), 0.25: (20, 10)}[thr]
    for k, (w, h) in enumerate((at, above)):
        bw, bh = big if k == 0 else ((20, 20) if thr == 0.6 else big)
        x0 = 100.0 + 200 * k
        rows.append(_xywh(x0, 100, x0 + bw, 100 + bh) + [0.9])            # the kept box ...
        rows.append(_xywh(x0, 100, x0 + w, 100 + h) + [0.8])              # ... and one inside it: IoU = its area / the big one's
    for nc, cls in ((1, 0), (3, 2)):
        pred = torch.zeros(1, 4, 5 + nc)
        pred[0, :, :5] = torch.tensor(rows)
        pred[0, :, 5 + cls] = 1.0
        ref = _check(oracle_mod, pred, conf=0.25, iou=thr, multi=False)
        assert ref[0].shape[0] == 3 and ref[0][:, 4].tolist() == [pytest.approx(0.9), pytest.approx(0.9), pytest.approx(0.8)]
        assert ref[0][2, 0] == 100.0                                  # the survivor is the one AT the threshold


def test_same_geometry_in_two_classes(oracle_mod):
    pred = torch.zeros(1, 3, 8)
    pred[0, :, :4] = torch.tensor([64.0, 64.0, 32.0, 32.0])
    pred[0, :, 4] = torch.tensor([0.9, 0.8, 0.7])
    pred[0, 0, 5], pred[0, 1, 7], pred[0, 2, 5] = 1.0, 1.0, 1.0
    assert _check(oracle_mod, pred, multi=False, agn=False)[0].shape[0] == 2    # classes 0 and 2; the second class-0 box goes
    assert _check(oracle_mod, pred, multi=False, agn=True)[0].shape[0] == 1
    assert _check(oracle_mod, pred, multi=True, agn=False)[0].shape[0] == 2


@pytest.mark.parametrize("seed", [0, 1, 2])
def test_random_sweep(oracle_mod, seed):
    rng = np.random.default_rng(1000 + seed)
    pred = _clustered(rng, 4, 2000, 3, centres=5 + seed)
    for multi, agn in ((True, False), (False, True)):
        ref = _check(oracle_mod, pred, conf=0.25, iou=0.45, multi=multi, agn=agn, max_det=300)
        cands = _yard(oracle_mod, pred, 0.25, 1.0, multi, agn, 10 ** 6)
        for r, c in zip(ref, cands):
            assert 1 < r.shape[0] < c.shape[0] and c.shape[0] > 1000    # suppressed and kept, in every image
    # more keys than one LDS tile of the sort (4096): the global passes
    cands = _yard(oracle_mod, pred, 0.001, 1.0, True, False, 10 ** 6)
    assert all(c.shape[0] > 4096 for c in cands)
    _check(oracle_mod, pred, conf=0.001, iou=0.6, multi=True, max_det=300)


def test_strided_input(oracle_mod):
    rng = np.random.default_rng(13)
    pred = _clustered(rng, 2, 150, 3)
    wide = torch.full((2, 150, 16), float("nan"), device=DEV)
    wide[:, :, :8] = pred.to(DEV)
    view = wide[:, :, :8]
    assert view.stride(1) == 16 and not view.is_contiguous()
    ref = _yard(oracle_mod, pred, 0.2, 0.5, True, False, 300)
    got, status = _device(view, 0.2, 0.5, True, False, 300)
    assert status == [0, 0]
    _same(got, ref)


def test_rows_past_the_end_are_untouched():
    from adaptiveisp_amd.yolo import _lib
    rng = np.random.default_rng(14)
    pred = _clustered(rng, 2, 100, 2).to(DEV)
    out = (torch.full((2 * 50, 6), -7.0, device=DEV), torch.full((3,), -7, dtype=torch.int32, device=DEV),
           torch.full((2,), -7, dtype=torch.int32, device=DEV))
    det, off, status = _lib.nms_batch(pred, 0.25, 0.45, 50, 30000, 200, True, False, out=out)
    k = int(off[2])
    assert 0 < k < 100 and bool((det[k:] == -7.0).all()) and status.tolist() == [0, 0] and int(off[0]) == 0


def test_graph_capture_and_replay(oracle_mod):
    """One call captured on one stream with preallocated outputs and workspace, replayed over two contents of `pred`."""
    from adaptiveisp_amd.yolo import _lib
    rng = np.random.default_rng(15)
    B, N, nc, max_det = 2, 300, 3, 40
    contents = [_clustered(rng, B, N, nc), _clustered(rng, B, N, nc, centres=3)]
    buf = contents[0].to(DEV)
    cap = N * nc
    ws = torch.empty(_lib.load().adayolo_nms_batch_workspace_bytes(B, N, nc, cap, 30000, max_det), dtype=torch.uint8, device=DEV)
    out = (torch.zeros(B * max_det, 6, device=DEV), torch.zeros(B + 1, dtype=torch.int32, device=DEV),
           torch.zeros(B, dtype=torch.int32, device=DEV))
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        _lib.nms_batch(buf, 0.2, 0.5, max_det, 30000, cap, True, False, workspace=ws, out=out)
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        _lib.nms_batch(buf, 0.2, 0.5, max_det, 30000, cap, True, False, workspace=ws, out=out)
    for content in (contents[1], contents[0]):
        buf.copy_(content)
        for t in out:
            t.fill_(-1)
        graph.replay()
        torch.cuda.synchronize()
        off = out[1].cpu().tolist()
        got = [out[0][off[b]:off[b + 1]].cpu() for b in range(B)]
        _same(got, _yard(oracle_mod, content, 0.2, 0.5, True, False, max_det))
        assert out[2].tolist() == [0, 0]


NC_EVAL = 4


class _TableDetector:
    """A detector stand-in a hipGraph can capture: per image a fixed table of rows in clusters around its labels (so that NMS
    suppresses), some strays, the second image of a batch with no candidate at all; every box shifted by a multiple of the
    retouched image's mean so that batches differ."""

    def __init__(self, B, H, W, seed):
        rng = np.random.default_rng(seed)
        self.labels = []
        table = np.zeros((B, 48, 5 + NC_EVAL), np.float32)
        for b in range(B):
            m = [3, 2, 4][b % 3]
            lab = np.concatenate([rng.integers(0, NC_EVAL, (m, 1)), rng.uniform(0.3, 0.7, (m, 2)), rng.uniform(0.15, 0.4, (m, 2))], 1)
            self.labels.append(lab)
            if b % 3 == 1:
                continue                                              # labels and no candidate
            for i in range(48):
                if i < 36:
                    k = i % m
                    table[b, i, :4] = lab[k, 1:] * (W, H, W, H) + rng.normal(0, 1.5, 4)
                    c = int(lab[k, 0]) if i % 3 else int(rng.integers(0, NC_EVAL))
                else:
                    table[b, i, :4] = (*rng.uniform(10, 80, 2), *rng.uniform(8, 30, 2))
                    c = int(rng.integers(0, NC_EVAL))
                table[b, i, 4] = rng.uniform(0.3, 0.95)
                table[b, i, 5:] = rng.uniform(0.0, 0.45, NC_EVAL)
                table[b, i, 5 + c] = rng.uniform(0.5, 0.95)
        self.table = torch.from_numpy(table).to(DEV)

    def __call__(self, x):
        shift = x.mean(dim=(1, 2, 3)) * 4.0
        out = self.table[:x.shape[0]].clone()
        out[:, :, :2] += shift[:, None, None]
        return out


@pytest.mark.parametrize("graph", [False, True])
@pytest.mark.parametrize("B", [1, 3])
def test_run_eval_device_nms_equals_host_nms(eval_agent, B, graph):
    """run_eval(match="device", nms="device") against run_eval(match="device"): the default NMS there is the HIP per-image path
    on device tensors, which the existing suite holds to the same oracle."""
    from adaptiveisp_amd.config import cfg
    from adaptiveisp_amd.val import run_eval
    H, W = 96, 128
    det = _TableDetector(B, H, W, seed=60 + B)
    shapes = [((H, W), ((1.0, 1.0), (0.0, 0.0))), ((192, 192), ((0.5, 0.5), (16.0, 0.0))), ((128, 256), ((0.5, 0.5), (0.0, 16.0))),
              ((192, 256), None)]
    g = torch.Generator().manual_seed(50)
    t = np.concatenate([np.concatenate([np.full((len(det.labels[b]), 1), b), det.labels[b]], 1) for b in range(B)])
    batches = [(torch.rand(B, 3, H, W, generator=g) * 0.6, torch.from_numpy(t.astype(np.float32)), [f"im{i}_{b}.png" for b in range(B)],
                [shapes[(i + b) % 4] for b in range(B)]) for i in range(3)]
    out = {}
    for mode in ("host", "device"):
        np.random.seed(3)
        details = []
        res = run_eval(eval_agent, det, batches, cfg, steps=2, conf_thres=0.2, nc=NC_EVAL, graph=graph, details=details,
                       match="device", nms=mode, confusion=True)
        out[mode] = (res, details)
    (rh, dh), (rd, dd) = out["host"], out["device"]
    assert rd["seen"] == 3 * B and rd["nms_fallbacks"] == 0 and rd["map50"] > 0
    _equal_results(rh, dh, rd, dd)
    kept = [d["pred"].shape[0] for d in dd]
    assert 0 < max(kept) < 48 * NC_EVAL and (B == 1 or 0 in kept)      # suppression happened; the empty image is there


def test_cli_device_nms_writes_the_same_files(tmp_path):
    """python -m adaptiveisp_amd.val --nms device (which implies --match device) against --match device alone."""
    from PIL import Image
    from _synth import synth_state_dict
    from adaptiveisp_amd.agent import Agent
    from adaptiveisp_amd.config import cfg
    os.makedirs(tmp_path / "data" / "images"); os.makedirs(tmp_path / "data" / "labels")
    rng = np.random.default_rng(21)
    for i, (h, w) in enumerate([(150, 200), (128, 96), (120, 120)]):
        im = np.kron(rng.random((h // 8 + 1, w // 8 + 1, 3)), np.ones((8, 8, 1)))[:h, :w] * 0.4 + rng.random((h, w, 3)) * 0.1
        Image.fromarray((im * 255).astype(np.uint8)).save(tmp_path / "data" / "images" / f"img{i}.png")
        lb = np.concatenate([rng.integers(0, 7, (2 + i, 1)).astype(np.float64), rng.uniform(0.25, 0.75, (2 + i, 2)),
                             rng.uniform(0.1, 0.4, (2 + i, 2))], 1)
        np.savetxt(tmp_path / "data" / "labels" / f"img{i}.txt", lb, fmt="%.6f")
    agent = Agent(cfg, shape=(6 + len(cfg.filters), 64, 64))
    torch.save({"iter": 0, "agent_model": synth_state_dict(agent, seed=0)}, tmp_path / "agent.pth")
    runs = {}
    for name, extra in (("match", ["--match", "device"]), ("nms", ["--nms", "device"])):
        cmd = ["timeout", "-k", "10", "300", sys.executable, "-m", "adaptiveisp_amd.val", "--isp-ckpt", str(tmp_path / "agent.pth"),
               "--detector-ckpt", os.path.join(GOLD, "yolov3_w0625_refpickle.pt"), "--data", str(tmp_path / "data" / "images"),
               "--img-size", "128", "--batch-size", "2", "--project", str(tmp_path / "runs"), "--name", name, "--confusion",
               "--save-txt", "--save-conf", "--graph", *extra]
        env = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
        r = subprocess.run(cmd, cwd=ROOT, env=env, capture_output=True, text=True)
        assert r.returncode == 0, f"exit {r.returncode}\n{r.stdout[-3000:]}\n{r.stderr[-3000:]}"
        runs[name] = (tmp_path / "runs" / name, r.stdout)
    assert "--match device" in runs["nms"][1]                         # the note that matching moved too
    a, b = runs["match"][0], runs["nms"][0]
    ra, rb = json.load(open(a / "results.json")), json.load(open(b / "results.json"))
    skip = ("ms_per_image", "args", "save_dir")
    assert {k: v for k, v in ra.items() if k not in skip} == {k: v for k, v in rb.items() if k not in skip}
    for f in ("records.txt", "confusion_matrix.csv"):
        assert (a / f).read_text() == (b / f).read_text(), f
    la, lb_ = sorted(os.listdir(a / "labels")), sorted(os.listdir(b / "labels"))
    assert la == lb_ and len(la) > 0
    for f in la:
        assert (a / "labels" / f).read_text() == (b / "labels" / f).read_text(), f
