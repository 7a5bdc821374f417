"""Detection metrics of the eval loop: IoU matrix, prediction/label matching at the 10 IoU levels, 101-point AP.

Same results as the reference's yolov3/utils/metrics.py (`ap_per_class` :31-96, `compute_ap` :98-123, `box_iou`
:262-280, `smooth` :21-28) and yolov3/val_adaptiveisp.py:79-103 (`process_batch`) — pinned bit-exactly by
tests/golden/evalharness.npz — but organised around what the computation IS rather than how the reference spells it:

  * matching: a detection can only ever be credited to its best same-class label (that pairing does not depend on the
    IoU level), and a label keeps the lowest-index detection that claims it — so all 10 levels come from one arg-max and
    one scatter-min instead of a per-level sort / unique / unique;
  * AP: detections are grouped by class with one stable sort; per-class cumulative TP/FP are segment cumsums over the
    whole array (exact integers), all IoU levels at once; only numpy's own interpolation runs per class;
  * confusion matrix (`ConfusionMatrix`, the reference's utils/metrics.py:126-184 without its plot): a detection claims its
    best label of ANY class, a label credits its best claimant — two arg-maxes instead of two sort / unique rounds.

`match_batch` / `ConfusionMatrix.process_batch_device` run the matching of a whole batch — the map to native image space, the
`correct` matrix at every level and the confusion counts — as one HIP launch (csrc/yolo_match.hip, `adayolo_match`).
"""
import numpy as np
import torch


def box_iou(box1, box2, eps=1e-7):
    """IoU matrix [N,M] of xyxy boxes (torch)."""
    lt = torch.maximum(box1[:, None, :2], box2[None, :, :2])
    rb = torch.minimum(box1[:, None, 2:4], box2[None, :, 2:4])
    wh = (rb - lt).clamp(min=0)
    inter = wh[..., 0] * wh[..., 1]
    area1 = (box1[:, 2] - box1[:, 0]) * (box1[:, 3] - box1[:, 1])
    area2 = (box2[:, 2] - box2[:, 0]) * (box2[:, 3] - box2[:, 1])
    return inter / (area1[:, None] + area2[None, :] - inter + eps)


def process_batch(detections, labels, iouv):
    """detections [N,6] (xyxy, conf, cls), labels [M,5] (cls, xyxy), iouv [T] ascending -> bool [N,T]: detection n counts
    as a true positive at level t.

    Rule (what the reference's sort-by-IoU + unique-by-detection + unique-by-label amounts to): detection d claims the
    same-class label with which it has the highest IoU, provided that IoU reaches the level; of the detections claiming
    one label, the one with the lowest index (= highest confidence after NMS) is credited."""
    N, M, T = detections.shape[0], labels.shape[0], iouv.shape[0]
    correct = torch.zeros((N, T), dtype=torch.bool, device=iouv.device)
    if N == 0 or M == 0:
        return correct
    iou = box_iou(labels[:, 1:], detections[:, :4])                                # [M,N]
    iou = torch.where(labels[:, 0:1] == detections[:, 5], iou, iou.new_full((), -1.0))
    best_iou, best_label = iou.max(dim=0)                                          # per detection
    claims = best_iou[:, None] >= iouv.to(best_iou.device)[None, :]                # [N,T]
    det_index = torch.arange(N, device=iou.device)[:, None].expand(N, T)
    first = torch.full((M, T), N, dtype=torch.int64, device=iou.device)
    first.scatter_reduce_(0, best_label[:, None].expand(N, T), torch.where(claims, det_index, N), reduce="amin")
    credited = claims & (first[best_label] == det_index)
    return credited.to(iouv.device)


def match_batch(det, det_offset, targets, geom, iouv, nc, native=False, confusion=None, cm_conf=0.25, cm_iou=0.45):
    """The matching of a whole batch as ONE launch of `adayolo_match` (HIP device tensors only; include/adayolo.h has the
    argument layout): det [K,6] post-NMS rows of all images, image-major; det_offset int32 [B+1]; targets [n,6] (image, class,
    x, y, w, h in network-input pixels, any row order); geom fp32 [B,5] (gain, pad_x, pad_y, h0, w0); iouv [T] on the device.
    -> (predn [K,6] native-space detections, correct uint8 [K,T]). `confusion`: an int32 [(nc+1)*(nc+1)] device tensor the
    confusion counts are ADDED to (ConfusionMatrix.process_batch_device hands over its own). `native`: boxes (det and target
    columns 2..5, xyxy) are in native space already — nothing is scaled or clipped, `geom` may be None."""
    from ..yolo import _lib
    return _lib.match(det, det_offset, targets, geom, iouv, nc, native=native, confusion=confusion, cm_conf=cm_conf,
                      cm_iou=cm_iou)


class ConfusionMatrix:
    """What the detector confuses with what: `matrix[p, t]` counts detections of class p credited to labels of class t, index
    `nc` being background — `matrix[nc, t]`: labels of class t nothing was credited to (missed), `matrix[p, nc]`: detections of
    class p credited to no label. Same counts as the reference's ConfusionMatrix.process_batch (utils/metrics.py:134-178).

    Rule, per image: of the detections with conf > `conf`, each claims the label it has the highest IoU with — whatever the
    classes — if that IoU is > `iou_thres`; a label credits the claimant with the highest IoU (matrix[det class, label class]
    += 1); a label nobody claims is a background miss; if the image has at least one claim, every kept detection that was not
    credited is a background prediction — with no claim at all the detections add nothing (the reference's behaviour, :166-178).

    Ties are OUR definition, not the reference's (which leaves them to numpy's unstable argsort()[::-1]): of equal IoUs the
    lowest label index, then the lowest detection index, wins.

    Counts made on the host (`process_batch`) and on the device (`process_batch_device`, inside the `adayolo_match` launch)
    add up in `.matrix`; the device counts are read back lazily, once, when `.matrix` is next asked for."""

    def __init__(self, nc, conf=0.25, iou_thres=0.45):
        self.nc, self.conf, self.iou_thres = int(nc), conf, iou_thres
        self._host = np.zeros((self.nc + 1, self.nc + 1), np.int64)
        self._dev = self._dev_host = None                    # int32 device counts; their host copy (None: stale)

    @property
    def matrix(self):
        """Integer [nc+1, nc+1], row = predicted, column = true, index nc = background (a copy: later counts do not
        change an array handed out earlier)."""
        if self._dev is None:
            return self._host.copy()
        if self._dev_host is None:
            self._dev_host = self._dev.cpu().numpy().astype(np.int64).reshape(self.nc + 1, self.nc + 1)
        return self._host + self._dev_host

    def process_batch(self, detections, labels):
        """detections [N,6] (xyxy, conf, class) or None, labels [M,5] (class, xyxy) in the same space — with
        `detections=None` a plain vector of label classes will do: every label is a background miss."""
        nc = self.nc
        labels = torch.as_tensor(labels).detach().cpu()
        if detections is None:
            gt = (labels[:, 0] if labels.ndim == 2 else labels).int().numpy()
            np.add.at(self._host, (nc, gt), 1)
            return
        detections = torch.as_tensor(detections).detach().cpu()
        detections = detections[detections[:, 4] > self.conf]
        N, M = detections.shape[0], labels.shape[0]
        gt, dc = labels[:, 0].int().numpy(), detections[:, 5].int().numpy()
        if M == 0:
            return
        if N == 0:
            np.add.at(self._host, (nc, gt), 1)
            return
        iou = box_iou(labels[:, 1:], detections[:, :4])                               # [M,N]
        best_iou = iou.max(dim=0).values                                              # per detection, over ALL labels
        label_index = torch.arange(M)[:, None].expand(M, N)
        best_label = torch.where(iou == best_iou[None, :], label_index, M).amin(dim=0)    # ties: lowest label index
        claims = best_iou > self.iou_thres
        # per label: the claimant with the highest IoU, ties to the lowest detection index
        top = torch.full((M,), -1.0).scatter_reduce_(0, best_label, torch.where(claims, best_iou, -1.0), reduce="amax")
        wins = claims & (best_iou == top[best_label])
        det_index = torch.arange(N)
        first = torch.full((M,), N, dtype=torch.int64).scatter_reduce_(0, best_label, torch.where(wins, det_index, N),
                                                                        reduce="amin")
        credited = (wins & (first[best_label] == det_index)).numpy()
        bl = best_label.numpy()
        np.add.at(self._host, (dc[credited], gt[bl[credited]]), 1)
        missed = np.ones(M, bool)
        missed[bl[credited]] = False
        np.add.at(self._host, (nc, gt[missed]), 1)
        if claims.any():
            np.add.at(self._host, (dc[~credited], nc), 1)

    def process_batch_device(self, det, det_offset, targets, geom, iouv, native=False):
        """A whole batch inside the matching launch (`match_batch`'s arguments): the counts are added to a device matrix of
        this object's. -> (predn, correct) as match_batch."""
        if self._dev is None or self._dev.device != det.device:
            if self._dev is not None:                        # counts made on another device move to the host side
                self._host = self.matrix.copy()
            self._dev = torch.zeros((self.nc + 1) * (self.nc + 1), dtype=torch.int32, device=det.device)
        self._dev_host = None
        return match_batch(det, det_offset, targets, geom, iouv, self.nc, native=native, confusion=self._dev,
                           cm_conf=self.conf, cm_iou=self.iou_thres)

    def tp_fp(self):
        """(true positives, false positives) per class, background left out."""
        m = self.matrix
        tp = m.diagonal()
        return tp[:-1], (m.sum(1) - tp)[:-1]

    def normalized(self):
        """Every column divided by its sum + 1e-9: what the reference's plot draws."""
        m = self.matrix
        return m / (m.sum(0).reshape(1, -1) + 1e-9)


def smooth(y, f=0.05):
    """Box filter over a fraction f of the curve, edges replicated."""
    nf = round(len(y) * f * 2) // 2 + 1            # odd window
    return np.convolve(np.pad(y, nf // 2, mode="edge"), np.full(nf, 1.0) / nf, mode="valid")


def _envelope(precision):
    """Monotone (non-increasing) envelope along axis 0: p'[i] = max(p[i:])."""
    return np.maximum.accumulate(precision[::-1], axis=0)[::-1]


_trapz = getattr(np, "trapezoid", None) or np.trapz          # numpy 2 renamed trapz
_GRID101 = np.linspace(0, 1, 101)


def compute_ap(recall, precision):
    """101-point interpolated AP (COCO style) of one precision/recall curve -> (ap, envelope precision, recall) with
    the sentinels (0,1) and (1,0) attached."""
    mrec = np.concatenate(([0.0], recall, [1.0]))
    mpre = _envelope(np.concatenate(([1.0], precision, [0.0])))
    return _trapz(np.interp(_GRID101, mrec, mpre), _GRID101), mpre, mrec


def ap_per_class(tp, conf, pred_cls, target_cls, eps=1e-16):
    """tp [n,T] bool, conf [n], pred_cls [n], target_cls [m] -> (tp, fp, p, r, f1, ap [nc,T], classes) over the
    classes present in the targets; p/r/f1 are taken at the confidence that maximises the smoothed mean F1."""
    classes, n_labels = np.unique(target_cls, return_counts=True)
    nc, T = classes.shape[0], tp.shape[1]
    grid = np.linspace(0, 1, 1000)
    ap, p_curve, r_curve = np.zeros((nc, T)), np.zeros((nc, 1000)), np.zeros((nc, 1000))
    # one ordering: by class, then by descending confidence inside a class
    by_conf = np.argsort(-conf)
    order = by_conf[np.argsort(pred_cls[by_conf], kind="stable")]
    cls_sorted, conf_sorted, hits = pred_cls[order], conf[order], tp[order].astype(np.int64)
    lo = np.searchsorted(cls_sorted, classes, side="left")
    hi = np.searchsorted(cls_sorted, classes, side="right")
    run = np.cumsum(hits, axis=0)                                   # running TP count over the whole ordering
    for ci in range(nc):
        a, b = lo[ci], hi[ci]
        if a == b or n_labels[ci] == 0:
            continue
        tpc = run[a:b] - (run[a - 1] if a else 0)                   # segment cumsum: TP so far inside this class
        fpc = np.arange(1, b - a + 1)[:, None] - tpc                # everything seen so far that was not a TP
        recall = tpc / (n_labels[ci] + eps)
        precision = tpc / (tpc + fpc)
        c = conf_sorted[a:b]
        r_curve[ci] = np.interp(-grid, -c, recall[:, 0], left=0)     # curves at IoU level 0 (mAP@0.5) over confidence
        p_curve[ci] = np.interp(-grid, -c, precision[:, 0], left=1)
        for j in range(T):
            ap[ci, j] = compute_ap(recall[:, j], precision[:, j])[0]
    f1_curve = 2 * p_curve * r_curve / (p_curve + r_curve + eps)
    k = smooth(f1_curve.mean(0), 0.1).argmax()
    p, r, f1 = p_curve[:, k], r_curve[:, k], f1_curve[:, k]
    tp_count = (r * n_labels).round()
    fp_count = (tp_count / (p + eps) - tp_count).round()
    return tp_count, fp_count, p, r, f1, ap, classes.astype(int)
