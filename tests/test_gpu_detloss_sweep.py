"""adayolo_detloss_fwd / _bwd (csrc/yolo_loss.hip) through the C-ABI against the float64 restatement tests/_detlossref.py
(pinned to the reference project's numbers by tests/test_detlossref_fixture.py), on hand-made match tables: the kernels never
see labels, so any geometry can sit on any cell. Class counts on both sides of the lane / lane + 64 split, pos_weight != 1,
label smoothing, every branch of the CIoU gradient (disjoint, nested, the four partial overlaps, extreme aspect ratios, tiny
targets, saturated sigmoids), cells matched up to 70 times, rows of no image, empty layers and images, a table read from
memory, ragged maps, channel strides wider than the maps.

Bounds (none comes from the kernels' output). e32 / e32_grad: the error of the fp32 CPU evaluation of the SAME restatement
against its float64 run on that case; 4x is the project's margin over a measured error (tools/set_tolerances.py).
  loss      |loss - ref64| <= 4 e32 + 4 * 2^-23 * max|ref64|   (the absolute term: four fp32 eps of the loss scale, for the
            cases where the fp32 run happens to land on the float64 value)
  gradient  |got - ref64| <= 2^-8 |ref64| + 4 e32_grad, every element: one bf16 ulp (half for the kernel's single rounding,
            half for a tie flipped by fp32 noise)
The four box-logit gradients of a cell whose CIoU sits within 1e-4 of a min / max / clamp switch are skipped (at most 5 % of
the matches, asserted); its class and objectness gradients are compared."""
import ctypes
import itertools

import numpy as np
import pytest
import torch

import _detlossref as R
import _margins

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
BF = torch.bfloat16
FILL = 0x7FC1                                       # bf16 NaN with a payload: the gradient buffers' content before the call
ANCHORS = torch.tensor([(1.25, 1.625), (2.0, 3.75), (4.125, 2.875), (0.3, 9.0)], dtype=torch.float64)
SIZES = {1: [(23, 40)], 3: [(64, 64), (23, 40), (3, 5)], 4: [(64, 64), (23, 40), (12, 7), (3, 5)]}
BALANCE = {1: [1.0], 3: [4.0, 1.0, 0.4], 4: [4.0, 1.0, 0.25, 0.06]}
WEIGHTS = [1.5, -0.25, 3.0, -2.0, 0.0625]           # upstream gradient of the per-image losses: mixed sign and magnitude


def bf(t):
    """Round a float64 tensor to bf16 values (kept as float64)."""
    return t.float().to(BF).double()


def f32(x):
    return float(np.float32(x))


def _u(g, n, lo, hi):
    return torch.rand(n, generator=g, dtype=torch.float64) * (hi - lo) + lo


def _sign(g, n):
    return torch.randint(0, 2, (n,), generator=g).double() * 2 - 1


# ---- geometry families: target boxes placed relative to the PREDICTED box of the cell (float64 decode of its bf16 logits)
def _anchors_for(family, n, g):
    if family == "aspect":                          # 1:30 and 30:1 predictions, alternating
        a = torch.tensor([(0.3, 9.0), (9.0, 0.3)], dtype=torch.float64)[torch.arange(n) % 2]
    elif family == "tiny":                          # every other match predicts a tiny box too
        a = ANCHORS[torch.randint(0, 4, (n,), generator=g)]
        a[0::2] = 0.0078125
    else:
        a = ANCHORS[torch.randint(0, 4, (n,), generator=g)]
    return bf(a)


def _logits_for(family, lg, g):
    """Box logits of the matched cells ([n,4], the map's randn * 3 draws), adjusted to the family."""
    n = lg.shape[0]
    if family == "saturated":
        mag = torch.tensor([8.0, 12.0, 20.0], dtype=torch.float64)[torch.randint(0, 3, (n, 4), generator=g)]
        sgn = torch.randint(0, 2, (n, 4), generator=g).double() * 2 - 1
        # a width saturated at 0 (w1 < 1e-5) is a degenerate box, within the kink margin of iwr = 0 whenever it lies inside
        # the target: 2 % of the rows keep such a size, the others saturate w and h at 4 anchors
        sgn[:, 2:] = torch.where(torch.rand(n, 1, generator=g) < 0.02, sgn[:, 2:], torch.ones(n, 2, dtype=torch.float64))
        return mag * sgn
    if family == "bulk":
        return lg
    lg = lg.clone()
    lg[:, 2:] = (lg[:, 2:] / (6.0 if family == "aspect" else 1.5)).clamp(-2, 2)      # crafted gaps are fractions of w1, h1
    return bf(lg)


def _targets_for(family, lg, anc, g, k0=0):
    """(tx, ty, tw, th) [n,4] in float64 for box logits lg and anchors anc; k0 shifts the sub-kind cycle."""
    n = lg.shape[0]
    q = R.geometry(lg, torch.cat([torch.ones(n, 4, dtype=torch.float64), anc], 1))
    x1, y1, w1, h1 = q["x1"], q["y1"], q["w1"], q["h1"]
    kind = (torch.arange(n) + k0) % 4
    if family in ("disj_x", "disj_y", "disj_xy"):
        w2, h2 = w1 * _u(g, n, 0.5, 1.5), h1 * _u(g, n, 0.5, 1.5)
        far_x = _sign(g, n) * (w1 + w2) / 2 * (1 + _u(g, n, 0.2, 1.0))
        far_y = _sign(g, n) * (h1 + h2) / 2 * (1 + _u(g, n, 0.2, 1.0))
        near_x, near_y = _u(g, n, -0.3, 0.3) * torch.minimum(w1, w2), _u(g, n, -0.3, 0.3) * torch.minimum(h1, h2)
        x2 = x1 + (near_x if family == "disj_y" else far_x)
        y2 = y1 + (near_y if family == "disj_x" else far_y)
    elif family == "pred_in_target":
        w2, h2 = w1 * _u(g, n, 1.5, 3.0), h1 * _u(g, n, 1.5, 3.0)
        x2, y2 = x1 + _u(g, n, -0.6, 0.6) * (w2 - w1) / 2, y1 + _u(g, n, -0.6, 0.6) * (h2 - h1) / 2
    elif family == "target_in_pred":
        w2, h2 = w1 * _u(g, n, 0.2, 0.6), h1 * _u(g, n, 0.2, 0.6)
        x2, y2 = x1 + _u(g, n, -0.6, 0.6) * (w1 - w2) / 2, y1 + _u(g, n, -0.6, 0.6) * (h1 - h2) / 2
    elif family == "partial":                       # the four corners the target can stick out of
        sx, sy = (kind % 2).double() * 2 - 1, (kind // 2).double() * 2 - 1
        w2, h2 = w1 * _u(g, n, 0.8, 1.25), h1 * _u(g, n, 0.8, 1.25)
        x2, y2 = x1 + sx * _u(g, n, 0.3, 0.7) * (w1 + w2) / 2, y1 + sy * _u(g, n, 0.3, 0.7) * (h1 + h2) / 2
    elif family == "aspect":                        # target 30:1 / 1:30 against a 1:30 / 30:1 prediction, and the same way round
        wide = (kind // 2 == 0) == (anc[:, 0] < anc[:, 1])
        short = _u(g, n, 0.25, 1.0)
        w2, h2 = torch.where(wide, 30 * short, short), torch.where(wide, short, 30 * short)
        x2, y2 = x1 + _u(g, n, -0.3, 0.3), y1 + _u(g, n, -0.3, 0.3)
    elif family == "tiny":                          # w2 h2 ~ 1e-4: the 1e-7 of the union matters
        w2, h2 = 0.01 * _u(g, n, 0.7, 1.4), 0.01 * _u(g, n, 0.7, 1.4)
        x2, y2 = x1 + _u(g, n, -0.3, 0.3) * torch.maximum(w1, w2), y1 + _u(g, n, -0.3, 0.3) * torch.maximum(h1, h2)
    else:                                           # bulk, saturated: the assignment's own ranges
        x2, y2 = _u(g, n, -0.5, 1.5), _u(g, n, -0.5, 1.5)
        w2, h2 = anc[:, 0] * 2 ** _u(g, n, -2, 2), anc[:, 1] * 2 ** _u(g, n, -2, 2)
    return bf(torch.stack((x2, y2, w2, h2), 1))


KINDS = {"disj_x": 1, "disj_y": 1, "disj_xy": 1, "pred_in_target": 1, "target_in_pred": 1, "partial": 4, "aspect": 4, "tiny": 2,
         "saturated": 3, "bulk": 2}


def _of_kind(family, q, lg, margin=R.KINK):
    """Per match: which of its family's KINDS sub-kinds it is (-1: none), from the float64 quantities."""
    iwr, ihr = q["iwr"], q["ihr"]
    none = torch.full(iwr.shape, -1, dtype=torch.long)
    pick = lambda cond, k=0: torch.where(cond, torch.full_like(none, k), none)          # noqa: E731
    m = margin
    if family == "disj_x":
        return pick((iwr < -m) & (ihr > m))
    if family == "disj_y":
        return pick((iwr > m) & (ihr < -m))
    if family == "disj_xy":
        return pick((iwr < -m) & (ihr < -m))
    inside = lambda a, b: ((q[f"l{b}"] < q[f"l{a}"] - m) & (q[f"r{a}"] < q[f"r{b}"] - m) & (q[f"t{b}"] < q[f"t{a}"] - m)   # noqa: E731
                           & (q[f"b{a}"] < q[f"b{b}"] - m))
    if family == "pred_in_target":
        return pick(inside(1, 2))
    if family == "target_in_pred":
        return pick(inside(2, 1))
    if family == "partial":
        ok = (iwr > m) & (ihr > m) & ((q["l1"] - q["l2"]).sign() == (q["r1"] - q["r2"]).sign()) \
            & ((q["t1"] - q["t2"]).sign() == (q["b1"] - q["b2"]).sign())
        return torch.where(ok, (q["r2"] > q["r1"]).long() + 2 * (q["b2"] > q["b1"]).long(), none)
    if family == "aspect":
        a1, a2 = q["w1"] / q["h1"], q["w2"] / q["h2"]
        ok = ((a1 < 1 / 12) | (a1 > 12)) & ((a2 < 1 / 25) | (a2 > 25))
        return torch.where(ok, (a1 > 1).long() + 2 * (a2 > 1).long(), none)
    if family == "tiny":
        ok = q["w2"] * q["h2"] < 3e-4
        return torch.where(ok, ((iwr > m) & (ihr > m)).long(), none)              # overlapping and not
    if family == "saturated":
        mag = lg.abs()
        ok = (mag >= 8).all(1)
        return torch.where(ok, (mag[:, 0] >= 12).long() + (mag[:, 0] >= 20).long(), none)
    return ((iwr > m) & (ihr > m)).long()                                             # bulk: disjoint and overlapping


# ---- cases ----------------------------------------------------------------------------------------------------------------
def _case(name, family, nc, na, nl, B, pw, smooth, cs="min", gcs="min", struct=(), n=300):
    return dict(name=name, family=family, nc=nc, na=na, nl=nl, B=B, pw=pw, cpcn=(0.95, 0.05) if smooth else (1.0, 0.0),
                cs=cs, gcs=gcs, struct=tuple(struct), n=n)


ALL = ("dups", "straddle", "ghost", "empty_image", "empty_layer")
CASES = [
    _case("bulk-nc80", "bulk", 80, 3, 3, 2, (1.0, 1.0), False),
    _case("bulk-nc1-dups", "bulk", 1, 3, 3, 5, (0.5, 2.0), False, gcs="wide", struct=("dups", "empty_image")),
    _case("bulk-nc128-fromMemory", "bulk", 128, 3, 1, 2, (3.0, 0.25), True, n=2500),
    _case("bulk-nc64-all", "bulk", 64, 1, 3, 5, (1.0, 1.0), True, cs="wide", struct=ALL),
    _case("bulk-nc2-nl4", "bulk", 2, 3, 4, 2, (3.0, 0.25), False, cs="wide", gcs="wide", struct=("ghost", "straddle")),
    _case("bulk-nc65-all", "bulk", 65, 3, 3, 2, (0.5, 2.0), True, struct=ALL),
    _case("disj_x-nc2", "disj_x", 2, 1, 1, 1, (3.0, 0.25), True, gcs="wide"),
    _case("disj_y-nc5", "disj_y", 5, 3, 4, 2, (0.5, 2.0), True, struct=("empty_layer", "empty_image")),
    _case("disj_xy-nc64", "disj_xy", 64, 3, 3, 2, (3.0, 0.25), False, cs="wide", struct=("ghost",)),
    _case("pred_in_target-nc65", "pred_in_target", 65, 3, 1, 5, (0.5, 2.0), True, struct=("straddle",)),
    _case("target_in_pred-nc128", "target_in_pred", 128, 1, 3, 2, (3.0, 0.25), True, gcs="wide"),
    _case("partial-nc80-dups", "partial", 80, 3, 3, 2, (0.5, 2.0), True, struct=("dups",)),
    _case("aspect-nc65", "aspect", 65, 1, 4, 1, (1.0, 1.0), True),
    _case("tiny-nc5", "tiny", 5, 3, 3, 2, (3.0, 0.25), False),
    _case("saturated-nc80", "saturated", 80, 3, 3, 2, (0.5, 2.0), True, struct=("dups",)),
]


def _stride(c, which):
    need = (c["na"] * (c["nc"] + 5) + 7) // 8 * 8          # the smallest multiple of 8 the argument check accepts
    return need if c[which] == "min" else max(need + 40, 256)


def build_case(c):
    """Host side of a case: bf16-exact float64 maps [B,na,ny,nx,no], per layer (idx int32 [n,5], box float64 [n,6], bf16-exact),
    and what the structure options planted. No GPU."""
    g = torch.Generator().manual_seed(sum(map(ord, c["name"])) * 7919 + 13)
    nc, na, nl, B, fam = c["nc"], c["na"], c["nl"], c["B"], c["family"]
    no = nc + 5
    images = B - 1 if "empty_image" in c["struct"] else B             # the last image gets no match in any layer
    assert images >= 1
    maps, tables, planted = [], [], {}
    for li, (ny, nx) in enumerate(SIZES[nl]):
        m = torch.randn(B, na, ny, nx, no, generator=g, dtype=torch.float64) * 4
        m[..., :4] *= 0.75                                           # box logits randn * 3
        flat = m.view(-1)
        pos = torch.randint(0, flat.numel(), (max(8, flat.numel() // 400),), generator=g)
        pos = pos[pos % no >= 4]                                     # a few +-30 among the class / objectness logits
        flat[pos] = 30.0 * _sign(g, pos.numel())
        m = bf(m)
        cells = images * na * ny * nx
        n = max(1, min(c["n"], cells // 2))
        if "empty_layer" in c["struct"] and li == nl - 1:
            n = 0
        pick = torch.randperm(cells, generator=g)[:n]                # distinct cells; duplicates are planted below
        b, r = pick // (na * ny * nx), pick % (na * ny * nx)
        a, r = r // (ny * nx), r % (ny * nx)
        gj, gi = r // nx, r % nx
        anc = _anchors_for(fam, n, g)
        m[b, a, gj, gi, :4] = _logits_for(fam, m[b, a, gj, gi, :4], g)
        box = torch.cat([_targets_for(fam, m[b, a, gj, gi, :4], anc, g), anc], 1)
        idx = torch.stack((b, a, gj, gi, torch.randint(0, nc, (n,), generator=g)), 1)
        if li == 0 and n:
            def more(rows, image_shift=0, want=None):                # further matches on the cells of `rows` (or of another image)
                i2 = idx[rows].clone()
                i2[:, 0] = (i2[:, 0] + image_shift) % images
                i2[:, 4] = torch.randint(0, nc, (len(rows),), generator=g)
                lg = m[i2[:, 0], i2[:, 1], i2[:, 2], i2[:, 3], :4]
                b2 = torch.cat([_targets_for(fam, lg, box[rows, 4:], g, k0=1), box[rows, 4:]], 1)
                if want is not None:                                 # keep rows whose branches are decided (reference quantities only)
                    ok = ~R.kink_mask(m, i2, b2)[0]
                    i2, b2 = i2[ok][:want], b2[ok][:want]
                    assert i2.shape[0] == want
                return i2, b2
            extra = []
            if "dups" in c["struct"]:                                # cells matched 2, 3 and 70 times
                clean = (~R.kink_mask(m, idx, box)[0]).nonzero().view(-1)
                r70 = int(clean[0])
                extra += [more([1 if r70 != 1 else 2]), more([3 if r70 != 3 else 4] * 2), more([r70] * 400, want=69)]
                planted["cell70"] = tuple(idx[r70, :4].tolist())
            if "straddle" in c["struct"] and images >= 2:            # the same (anchor, gj, gi) in two images, twice each
                extra += [more([5, 6, 7]), more([5, 6, 7], image_shift=1), more([5, 6, 7], image_shift=1)]
                planted["straddle"] = [tuple(idx[k, 1:4].tolist()) for k in (5, 6, 7)]
            if extra:
                idx = torch.cat([idx] + [e[0] for e in extra])
                box = torch.cat([box] + [e[1] for e in extra])
                order = torch.randperm(idx.shape[0], generator=g)    # the planted rows end up anywhere in the table
                idx, box = idx[order], box[order]
            if "ghost" in c["struct"]:                               # rows of image -1 and B in front of every other row
                k = idx.shape[0] // 2
                gh = idx[0::2][:k].clone()
                gh[:, 0] = torch.where(torch.arange(k) % 2 == 0, -1, B)
                n2 = idx.shape[0] + k
                where = torch.zeros(n2, dtype=torch.bool)
                where[0:3 * k:3] = True
                i3, b3 = torch.zeros(n2, 5, dtype=idx.dtype), torch.zeros(n2, 6, dtype=box.dtype)
                i3[where], b3[where] = gh, box[0::2][:k]
                i3[~where], b3[~where] = idx, box
                idx, box = i3, b3
                planted["ghosts"] = k
        maps.append(m)
        tables.append((idx.to(torch.int32).contiguous(), box.contiguous()))
    for m, (idx, box) in zip(maps, tables):                           # everything handed to the kernels is bf16-exact
        assert torch.equal(bf(m), m) and torch.equal(bf(box), box)
    return maps, tables, planted


def hyper(c):
    return dict(balance=[f32(x) for x in BALANCE[c["nl"]]], hyp_box=f32(0.05), hyp_obj=f32(0.7), hyp_cls=f32(0.3),
                cp=f32(c["cpcn"][0]), cn=f32(c["cpcn"][1]), cls_pw=f32(c["pw"][0]), obj_pw=f32(c["pw"][1]), nc=c["nc"])


def reference(c, maps, tables):
    """float64 and float32 CPU runs of the restatement, the kink masks and the per-case conditions that need no GPU."""
    hyp, B = hyper(c), c["B"]
    w = WEIGHTS[:B]
    l64, g64 = R.loss_and_grads(maps, tables, w, **hyp)
    l32, g32 = R.loss_and_grads([m.float() for m in maps], [(i, b.float()) for i, b in tables], w, **hyp)
    masks = [R.kink_mask(m, idx, box) for m, (idx, box) in zip(maps, tables)]
    total = sum(int(pm.numel()) for pm, _ in masks)
    share = sum(int(pm.sum()) for pm, _ in masks) / max(total, 1)
    # every sub-kind of the family keeps unmasked matches (per match AND per cell: a masked cell's box gradients are skipped)
    seen = set()
    for m, (idx, box), (pm, cells) in zip(maps, tables, masks):
        keep, b, a, gj, gi, _ = R._rows(idx, B)
        if not int(b.shape[0]):
            continue
        lg = m[b, a, gj, gi, :4]
        kind = _of_kind(c["family"], R.geometry(lg, box[keep]), lg)
        free = ~pm & ~cells[b, a, gj, gi]
        seen |= set(kind[free & (kind >= 0)].tolist())
    return dict(l64=l64, g64=g64, l32=l32, g32=g32, masks=masks, share=share, total=total, kinds=seen)


def _launch(c, maps, tables, lib, L):
    """One forward + backward on fresh buffers. Returns (loss [B] fp32, gradient buffers [B,ny,nx,grad_cs] bf16, ticket), on the CPU."""
    B, na, nc, nl = c["B"], c["na"], c["nc"], c["nl"]
    no, cs, gcs = nc + 5, _stride(c, "cs"), _stride(c, "gcs")
    a, keep, grads = lib.LossArgs(), [], []
    g = torch.Generator().manual_seed(5)
    hyp = hyper(c)
    for i, (m, (idx, box)) in enumerate(zip(maps, tables)):
        ny, nx = m.shape[2], m.shape[3]
        raw = torch.randn(B, ny, nx, cs, generator=g).to(BF)                          # junk beyond na * no: never read
        raw[..., : na * no] = m.permute(0, 2, 3, 1, 4).reshape(B, ny, nx, na * no).to(BF)
        raw = raw.to(DEV)
        grad = torch.full((B, ny, nx, gcs), FILL, dtype=torch.int16, device=DEV).view(BF)
        nan = float("nan")
        ws = [torch.full((B, 3), nan, device=DEV), torch.full((B, na, ny, nx), nan, device=DEV), torch.full((B,), nan, device=DEV)]
        n = int(idx.shape[0])
        ok = (idx[:, 0] >= 0) & (idx[:, 0] < B)                                        # bounds of every row a kernel dereferences
        lim = torch.tensor([B, na, ny, nx, nc])
        assert ((idx[ok] >= 0) & (idx[ok] < lim)).all()
        d_idx, d_box = idx.to(DEV), box.float().contiguous().to(DEV)
        assert d_idx.dtype == torch.int32 and d_idx.is_contiguous() and d_box.shape == (n, 6)
        Ly = a.layer[i]
        Ly.raw, Ly.cs, Ly.ny, Ly.nx, Ly.balance = raw.data_ptr(), cs, ny, nx, hyp["balance"][i]
        Ly.idx, Ly.box, Ly.n = (d_idx.data_ptr() if n else None), (d_box.data_ptr() if n else None), n
        Ly.part, Ly.tobj, Ly.cnt = ws[0].data_ptr(), ws[1].data_ptr(), ws[2].data_ptr()
        Ly.grad, Ly.grad_cs = grad.data_ptr(), gcs
        grads.append(grad)
        keep += ws + [raw, d_idx, d_box]
    a.nl, a.B, a.na, a.nc, a.no = nl, B, na, nc, no
    a.hyp_box, a.hyp_obj, a.hyp_cls = hyp["hyp_box"], hyp["hyp_obj"], hyp["hyp_cls"]
    a.cp, a.cn, a.cls_pw, a.obj_pw = hyp["cp"], hyp["cn"], hyp["cls_pw"], hyp["obj_pw"]
    loss = torch.full((B,), float("nan"), device=DEV)
    ticket = torch.zeros((B,), dtype=torch.int32, device=DEV)
    w = torch.tensor(WEIGHTS[:B], device=DEV)
    a.loss, a.ticket, a.grad_loss = loss.data_ptr(), ticket.data_ptr(), w.data_ptr()
    st = lib.stream_ptr()
    lib.check(L.adayolo_detloss_fwd(ctypes.byref(a), st), "adayolo_detloss_fwd")
    lib.check(L.adayolo_detloss_bwd(ctypes.byref(a), st), "adayolo_detloss_bwd")
    torch.cuda.synchronize()
    return loss.cpu(), [x.cpu() for x in grads], ticket.cpu()


def _bits(t):
    return t.view(torch.int16)


@pytest.mark.parametrize("c", CASES, ids=[c["name"] for c in CASES])
def test_detloss_kernels_against_float64(c):
    from adaptiveisp_amd.yolo import _lib
    L = _lib.load()
    B, na, nc = c["B"], c["na"], c["nc"]
    no = nc + 5
    maps, tables, planted = build_case(c)
    ref = reference(c, maps, tables)
    name = c["name"]
    # conditions on the case itself (reference quantities only)
    print(f"{name}: {ref['total']} matches, kinked-out share {ref['share']:.4f}, kinds seen {sorted(ref['kinds'])}")
    assert ref["share"] <= 0.05, ref["share"]
    assert ref["kinds"] >= set(range(KINDS[c["family"]])), ref["kinds"]
    if c["n"] > 2048:
        assert tables[0][0].shape[0] > 2048                          # the kernels read this table from memory
    if "cell70" in planted:                                          # 70 matches of one cell, more than 64 rows apart, box gradients compared
        idx0 = tables[0][0].long()
        rows = (idx0[:, :4] == torch.tensor(planted["cell70"])).all(1).nonzero().view(-1)
        assert rows.numel() == 70 and int(rows[-1] - rows[0]) >= 64
        assert not ref["masks"][0][1][planted["cell70"]]
        per_cell = {}
        for r in idx0[:, :4].tolist():
            per_cell[tuple(r)] = per_cell.get(tuple(r), 0) + 1
        assert {2, 3, 70} <= set(per_cell.values())
    if "ghosts" in planted:
        col = tables[0][0][:, 0]
        assert int((col == -1).sum()) > 0 and int((col == B).sum()) > 0
    if "empty_image" in c["struct"]:
        assert all(int((idx[:, 0] == B - 1).sum()) == 0 for idx, _ in tables)
    if "empty_layer" in c["struct"]:
        assert tables[-1][0].shape[0] == 0

    loss, grads, ticket = _launch(c, maps, tables, _lib, L)
    loss2, grads2, ticket2 = _launch(c, maps, tables, _lib, L)

    # loss
    e32 = float((ref["l32"].double() - ref["l64"]).abs().max())
    atol = 4 * 2.0 ** -23 * float(ref["l64"].abs().max())
    err = float((loss.double() - ref["l64"]).abs().max())
    print(f"{name}: loss err {err:.3e}  e32 {e32:.3e}  bound {4 * e32 + atol:.3e}")
    notes = [f"detloss_sweep {name}: loss err {err:.3e} (e32 {e32:.3e}, asserted {4 * e32 + atol:.3e})"]
    failures = []
    try:
        _margins.close(f"detloss_sweep:loss:{name}", loss.double(), ref["l64"], rtol=0.0, atol=4 * e32 + atol)
    except AssertionError as e:
        failures.append(str(e))

    # gradient maps
    stride_nano = na * no
    for i, (gr, m, (idx, box)) in enumerate(zip(grads, maps, tables)):
        ny, nx = m.shape[2], m.shape[3]
        assert not (_bits(gr) == FILL).any(), f"layer {i}: fill value left in the gradient buffer"
        assert (_bits(gr)[..., stride_nano:] == 0).all(), f"layer {i}: channels beyond na * no are not zero"
        got = gr[..., :stride_nano].double().view(B, ny, nx, na, no).permute(0, 3, 1, 2, 4)
        gotbits = _bits(gr)[..., :stride_nano].reshape(B, ny, nx, na, no).permute(0, 3, 1, 2, 4)
        want, want32 = ref["g64"][i], ref["g32"][i].double()
        keep = torch.ones_like(want, dtype=torch.bool)
        keep[..., :4] &= ~ref["masks"][i][1][..., None]              # the box logits of the kinked cells, nothing else
        e32g = float((want32 - want).abs()[keep].max())
        errg = float((got - want).abs()[keep].max())
        print(f"{name} layer {i}: grad err {errg:.3e}  e32_grad {e32g:.3e}  max|ref| {float(want.abs().max()):.3e}")
        notes.append(f"detloss_sweep {name} layer {i}: grad err {errg:.3e} (e32_grad {e32g:.3e}, max |ref| {float(want.abs().max()):.3e})")
        try:
            _margins.close(f"detloss_sweep:grad:{name}", got[keep], want[keep], rtol=2.0 ** -8, atol=4 * e32g)
        except AssertionError as e:
            bad = ((got - want).abs() > 2.0 ** -8 * want.abs() + 4 * e32g) & keep
            where = bad.nonzero()[:5].tolist()
            failures.append(f"layer {i}: {e}; {int(bad.sum())} elements, first at (b, a, gj, gi, ch) {where}")
        # cells no match touches: exactly zero but the objectness channel, which holds bf16(dense term): w_b hyp_obj balance /
        # cells * sigmoid(x) at target 0. The fp32 evaluation (three products, expf, an add, a division: <= 2^-18 relative;
        # 1 - (1 - sigmoid) loses sigmoid below 2^-24: 2^-23 of the factor in front) lies in [lo, hi]; rounding is monotone
        keep_rows, b, a_, gj, gi, _ = R._rows(idx, B)
        touched = torch.zeros(B, na, ny, nx, dtype=torch.bool)
        touched[b, a_, gj, gi] = True
        other = torch.ones(no, dtype=torch.bool)
        other[4] = False
        assert (gotbits[~touched][:, other] == 0).all(), f"layer {i}: an unmatched cell has a box / class gradient"
        front = torch.tensor(WEIGHTS[:B], dtype=torch.float64).abs() * hyper(c)["hyp_obj"] * hyper(c)["balance"][i] / (na * ny * nx)
        tol = 2.0 ** -18 * want[..., 4].abs() + 2.0 ** -23 * front.view(B, 1, 1, 1)
        lo, hi = bf(want[..., 4] - tol), bf(want[..., 4] + tol)
        dense_ok = (got[..., 4] >= lo) & (got[..., 4] <= hi)
        if not dense_ok[~touched].all():
            failures.append(f"layer {i}: {int((~dense_ok[~touched]).sum())} unmatched cells do not hold bf16(dense objectness term)")
        assert torch.equal(_bits(gr), _bits(grads2[i])), f"layer {i}: the second run's gradient differs"
    _margins.NOTES.extend(notes)
    assert (ticket == 0).all() and (ticket2 == 0).all()
    assert torch.equal(loss.view(torch.int32), loss2.view(torch.int32)), "the second run's loss differs"
    assert not failures, "\n".join(failures)


def test_more_than_two_classes_per_lane_is_refused():
    """nc = 129 (tests/test_cabi.py has 200): ADAYOLO_ESHAPE before any launch."""
    from adaptiveisp_amd.yolo import _lib
    L = _lib.load()
    buf = torch.zeros(4096, device=DEV)
    p = buf.data_ptr()
    a = _lib.LossArgs()
    a.nl, a.B, a.na, a.nc, a.no, a.loss, a.ticket, a.grad_loss = 1, 1, 1, 129, 134, p + 4224, p + 4288, p + 4352
    lay = a.layer[0]
    lay.raw, lay.cs, lay.ny, lay.nx, lay.n, lay.grad, lay.grad_cs = p, 136, 2, 2, 0, p + 8192, 136       # (disjoint byte ranges)
    lay.tobj, lay.cnt, lay.part = p + 2048, p + 4096, p + 4160
    assert L.adayolo_detloss_fwd(ctypes.byref(a), None) == -2 and L.adayolo_detloss_bwd(ctypes.byref(a), None) == -2
    a.nc, a.no = 128, 133                                           # the largest class count passes the check
    assert L.adayolo_detloss_fwd(ctypes.byref(a), _lib.stream_ptr()) == 0
    torch.cuda.synchronize()


def test_case_table_covers_what_it_claims():
    """The parameter values the sweep is meant to reach are in the case table (a case dropped by accident would go unnoticed)."""
    col = lambda k: {c[k] for c in CASES}                              # noqa: E731
    assert col("nc") >= {1, 2, 5, 64, 65, 80, 128} and col("na") == {1, 3} and col("nl") == {1, 3, 4} and col("B") == {1, 2, 5}
    assert col("pw") == {(1.0, 1.0), (0.5, 2.0), (3.0, 0.25)} and col("cpcn") == {(1.0, 0.0), (0.95, 0.05)}
    assert col("family") == {"bulk", "disj_x", "disj_y", "disj_xy", "pred_in_target", "target_in_pred", "partial", "aspect", "tiny",
                             "saturated"}
    assert col("cs") == {"min", "wide"} and any(_stride(c, "cs") != _stride(c, "gcs") for c in CASES)
    assert set(itertools.chain.from_iterable(c["struct"] for c in CASES)) == set(ALL) and any(c["n"] > 2048 for c in CASES)
