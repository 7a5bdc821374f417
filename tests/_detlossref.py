"""Plain-torch restatement of the per-image detection loss that csrc/yolo_loss.hip documents, on the kernels' OWN inputs
(head maps + the packed match tables, not labels), in whatever dtype the maps have: float64 is the reference of
tests/test_gpu_detloss_sweep.py, the float32 run of the same function is the yardstick for its bounds.
tests/test_detlossref_fixture.py pins it to the reference project's numbers (tests/golden/detloss.npz).

Per layer i, image b (rows of `idx` whose image index is outside [0, B) belong to no image):
  pxy = 2 sigmoid - 0.5, pwh = (2 sigmoid)^2 anchor, CIoU against the target box (alpha under no_grad),
  lbox_b = mean over b's matches of 1 - CIoU,  lcls_b = mean over (b's matches) x nc of BCE (dropped when nc == 1),
  tobj[cell] = clamp(CIoU, 0) of the LAST match of the cell (an explicit sequential loop, never index_put_),
  lobj_b = mean over b's (na, ny, nx) cells of BCE * balance_i,
loss_b = hyp_box sum_i lbox + hyp_obj sum_i lobj + hyp_cls sum_i lcls. Test infrastructure only."""
import math

import torch
import torch.nn.functional as F

EPS = 1e-7
KINK = 1e-4          # a branch-deciding quantity closer than this to its switch: the box-logit gradients of the cell are not compared


def _rows(idx, B):
    """Rows of the match table that belong to an image, in table order: (keep mask, b, a, gj, gi, cls) as int64."""
    idx = torch.as_tensor(idx).long().reshape(-1, 5)
    keep = (idx[:, 0] >= 0) & (idx[:, 0] < B)
    b, a, gj, gi, c = idx[keep].T
    return keep, b, a, gj, gi, c


def geometry(lg, box):
    """Every quantity of the CIoU of the predicted box (box logits lg [n,4], anchor box[:, 4:6]) against the target
    box[:, :4], in lg's dtype, as a dict of [n] tensors."""
    box = box.to(lg.dtype)
    s = lg.sigmoid()
    x1, y1 = s[:, 0] * 2 - 0.5, s[:, 1] * 2 - 0.5
    w1, h1 = (s[:, 2] * 2) ** 2 * box[:, 4], (s[:, 3] * 2) ** 2 * box[:, 5]
    x2, y2, w2, h2 = box[:, 0], box[:, 1], box[:, 2], box[:, 3]
    q = dict(x1=x1, y1=y1, w1=w1, h1=h1, x2=x2, y2=y2, w2=w2, h2=h2)
    q.update(l1=x1 - w1 / 2, r1=x1 + w1 / 2, t1=y1 - h1 / 2, b1=y1 + h1 / 2)
    q.update(l2=x2 - w2 / 2, r2=x2 + w2 / 2, t2=y2 - h2 / 2, b2=y2 + h2 / 2)
    q["iwr"] = torch.minimum(q["r1"], q["r2"]) - torch.maximum(q["l1"], q["l2"])
    q["ihr"] = torch.minimum(q["b1"], q["b2"]) - torch.maximum(q["t1"], q["t2"])
    return q


def ciou(lg, box):
    q = geometry(lg, box)
    inter = q["iwr"].clamp(min=0) * q["ihr"].clamp(min=0)
    union = q["w1"] * q["h1"] + q["w2"] * q["h2"] - inter + EPS
    iou = inter / union
    cw = torch.maximum(q["r1"], q["r2"]) - torch.minimum(q["l1"], q["l2"])
    ch = torch.maximum(q["b1"], q["b2"]) - torch.minimum(q["t1"], q["t2"])
    c2 = cw ** 2 + ch ** 2 + EPS
    rho2 = ((q["l2"] + q["r2"] - q["l1"] - q["r1"]) ** 2 + (q["t2"] + q["b2"] - q["t1"] - q["b1"]) ** 2) / 4
    v = (4 / math.pi ** 2) * (torch.atan(q["w2"] / q["h2"]) - torch.atan(q["w1"] / q["h1"])) ** 2
    with torch.no_grad():
        alpha = v / (v - iou + (1 + EPS))
    return iou - (rho2 / c2 + v * alpha)


def per_image_loss(maps, tables, *, balance, hyp_box, hyp_obj, hyp_cls, cp, cn, cls_pw, obj_pw, nc):
    """maps: per layer [B, na, ny, nx, 5 + nc]; tables: per layer (idx int [n,5] = (image, anchor, gj, gi, class),
    box [n,6] = (tx, ty, tw, th, anchor_w, anchor_h)). Returns loss [B] in the maps' dtype."""
    dt, B = maps[0].dtype, maps[0].shape[0]
    total = torch.zeros(B, dtype=dt)
    for pi, (idx, box), bal in zip(maps, tables, balance):
        assert pi.shape[4] == 5 + nc and pi.dtype == dt
        tobj = torch.zeros(pi.shape[:4], dtype=dt)
        keep, b, a, gj, gi, c = _rows(idx, B)
        n = int(b.shape[0])
        if n:
            box = torch.as_tensor(box).reshape(-1, 6)[keep].to(dt)
            cell = pi[b, a, gj, gi]                                         # [n, no]
            iou = ciou(cell[:, :4], box)
            cnt = torch.zeros(B, dtype=dt).index_add_(0, b, torch.ones(n, dtype=dt))
            inv = torch.where(cnt > 0, 1.0 / cnt.clamp(min=1.0), torch.zeros_like(cnt))
            total = total + hyp_box * torch.zeros(B, dtype=dt).index_add(0, b, 1.0 - iou) * inv
            tv = iou.detach().clamp(min=0)
            for j, (bb, aa, yy, xx) in enumerate(zip(b.tolist(), a.tolist(), gj.tolist(), gi.tolist())):
                tobj[bb, aa, yy, xx] = tv[j]                                # in table order: the last match of a cell wins
            if nc > 1:
                t = torch.full((n, nc), cn, dtype=dt)
                t[torch.arange(n), c] = cp
                bce = F.binary_cross_entropy_with_logits(cell[:, 5:], t, reduction="none",
                                                         pos_weight=torch.tensor([cls_pw], dtype=dt))
                total = total + hyp_cls * torch.zeros(B, dtype=dt).index_add(0, b, bce.sum(1)) * inv / nc
        obj = F.binary_cross_entropy_with_logits(pi[..., 4], tobj, reduction="none", pos_weight=torch.tensor([obj_pw], dtype=dt))
        total = total + hyp_obj * bal * obj.mean(dim=(1, 2, 3))
    return total


def loss_and_grads(maps, tables, weights, **hyp):
    """(loss [B], [d sum_b w_b loss_b / d map] per layer) by autograd, in the maps' dtype."""
    leaves = [m.detach().clone().requires_grad_(True) for m in maps]
    loss = per_image_loss(leaves, tables, **hyp)
    (loss * torch.as_tensor(weights).to(loss.dtype)).sum().backward()
    return loss.detach(), [m.grad if m.grad is not None else torch.zeros_like(m) for m in leaves]


def kink_quantities(pi, idx, box):
    """The float64 quantities that decide a branch of the CIoU gradient, per match that belongs to an image: [n, 6] =
    (r1 - r2, l1 - l2, t1 - t2, b1 - b2, iwr, ihr), with the rows' (keep, b, a, gj, gi)."""
    keep, b, a, gj, gi, _ = _rows(idx, pi.shape[0])
    if int(b.shape[0]) == 0:
        return torch.zeros((0, 6), dtype=torch.float64), (keep, b, a, gj, gi)
    q = geometry(pi.detach().double()[b, a, gj, gi][:, :4], torch.as_tensor(box).reshape(-1, 6)[keep].double())
    k = torch.stack((q["r1"] - q["r2"], q["l1"] - q["l2"], q["t1"] - q["t2"], q["b1"] - q["b2"], q["iwr"], q["ihr"]), 1)
    return k, (keep, b, a, gj, gi)


def kink_mask(pi, idx, box, margin=KINK):
    """Per match that belongs to an image (table order): True where min / max / clamp(0) of the CIoU switches within
    `margin` of the float64 value, so fp32 arithmetic may take the other branch. Also the [B, na, ny, nx] mask of the
    cells such a match sits on: their four box-logit gradients, and nothing else, are left out of a comparison."""
    k, (_, b, a, gj, gi) = kink_quantities(pi, idx, box)
    per_match = (k.abs() < margin).any(1)
    cells = torch.zeros(pi.shape[:4], dtype=torch.bool)
    cells[b[per_match], a[per_match], gj[per_match], gi[per_match]] = True
    return per_match, cells
