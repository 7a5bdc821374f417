"""tests/_detlossref.py (the float64 reference of tests/test_gpu_detloss_sweep.py) pinned to the reference project's own
numbers: detloss.npz `q*` — bf16-exact head maps scored by its ComputeLossBatch one sample at a time, with autograd's
gradient of sum_b w_b loss_b. Without this pin the GPU sweep would compare the kernels against an unanchored formula."""
import numpy as np
import torch

import _detlossref

EPS32 = 2.0 ** -23


def _fixture(golden):
    from adaptiveisp_amd.yolo.loss import DetectionLoss, pack_assigned
    g = golden("detloss")
    # the hyper-parameters of test_detloss_kernels_against_the_reference_fixture_directly
    hyp = dict(box=0.05, cls=0.5, obj=1.0 * (96 / 640) ** 2, anchor_t=4.0, cls_pw=1.0, obj_pw=1.0, fl_gamma=0.0,
               label_smoothing=0.0)
    loss_fn = DetectionLoss(torch.from_numpy(g["anchors"]), nc=80, hyp=hyp, device="cpu")
    qs = [torch.from_numpy(g[f"q{i}"]) for i in range(3)]
    tables = pack_assigned(loss_fn.assign(qs, torch.from_numpy(g["targets"])))
    kw = dict(balance=loss_fn.balance, hyp_box=hyp["box"], hyp_obj=hyp["obj"], hyp_cls=hyp["cls"], cp=loss_fn.cp, cn=loss_fn.cn,
              cls_pw=1.0, obj_pw=1.0, nc=80)
    return g, qs, tables, kw


def test_float64_restatement_reproduces_the_fixture(golden):
    g, qs, tables, kw = _fixture(golden)
    B = qs[0].shape[0]
    assert sum(int(idx.shape[0]) for idx, _ in tables) == 68            # the matches the issue counts
    loss, grads = _detlossref.loss_and_grads([q.double() for q in qs], tables, g["qweights"], **kw)
    want = np.array([g[f"qsample{b}"].astype(np.float64).sum() for b in range(B)])
    # The fixture is fp32 arithmetic, the restatement float64: 4 fp32 eps of each tensor's scale are asserted. Needed
    # (measured on the CPU): the losses 0.33 eps of their scale, the gradient maps 3.6 / 2.7 / 1.9 eps of theirs (the
    # fixture's own fp32 rounding: the fp32 run of the restatement, next test, is held to 8 eps of the float64 one).
    err = np.abs(loss.numpy() - want)
    print("loss err / eps32 / scale:", err.max() / EPS32 / np.abs(want).max())
    assert (err <= 4 * EPS32 * np.abs(want).max()).all(), (loss.numpy(), want)
    for i, gr in enumerate(grads):
        ref = g[f"qgrad{i}"].astype(np.float64)
        scale = np.abs(ref).max()
        e = np.abs(gr.numpy() - ref).max()
        print(f"qgrad{i} err / eps32 / scale:", e / EPS32 / scale)
        assert e <= 4 * EPS32 * scale, (i, e, scale)


def test_float32_run_is_the_same_function(golden):
    """The fp32 evaluation (the yardstick of the sweep's bounds) differs from the float64 one by fp32 rounding only."""
    g, qs, tables, kw = _fixture(golden)
    l64, g64 = _detlossref.loss_and_grads([q.double() for q in qs], tables, g["qweights"], **kw)
    l32, g32 = _detlossref.loss_and_grads(qs, tables, g["qweights"], **kw)
    assert l32.dtype == torch.float32 and all(x.dtype == torch.float32 for x in g32)
    assert ((l32.double() - l64).abs() <= 8 * EPS32 * l64.abs().max()).all()
    for a, b in zip(g32, g64):
        assert (a.double() - b).abs().max() <= 8 * EPS32 * b.abs().max()


def test_rows_of_no_image_and_the_last_match(golden):
    """Rows with image index -1 / B change nothing; of two matches on one cell the later one sets the objectness target."""
    g, qs, tables, kw = _fixture(golden)
    qs = [q.double() for q in qs]
    B = qs[0].shape[0]
    base = _detlossref.per_image_loss(qs, tables, **kw)
    ghost = []
    for idx, box in tables:
        gi = idx.clone().repeat_interleave(2, 0)                 # a copy in front of every row, as a row of image -1 / B
        gi[0::2, 0] = torch.where(torch.arange(idx.shape[0]) % 2 == 0, -1, B).to(gi.dtype)
        ghost.append((gi, box.repeat_interleave(2, 0)))
    assert torch.equal(_detlossref.per_image_loss(qs, ghost, **kw), base)
    idx, box = tables[0]
    two = (torch.cat([idx[:1], idx[:1]]), torch.cat([box[:1], box[:1] * torch.tensor([1, 1, 0.5, 0.5, 1, 1])]))
    swapped = (two[0], two[1].flip(0))
    one = [two] + [(t[0][:0], t[1][:0]) for t in tables[1:]]
    other = [swapped] + one[1:]
    assert not torch.equal(_detlossref.per_image_loss(qs, one, **kw), _detlossref.per_image_loss(qs, other, **kw))


def test_kink_mask_marks_the_switches():
    pi = torch.zeros(1, 1, 1, 2, 6, dtype=torch.float64)        # logits 0: x1 = y1 = 0.5, w1 = h1 = anchor
    idx = torch.tensor([[0, 0, 0, 0, 0], [0, 0, 0, 1, 0], [1, 0, 0, 0, 0]])
    box = torch.tensor([[0.5, 0.5, 2.0 + 1e-5, 3.0, 2.0, 1.0],      # r1 - r2 = -5e-6: masked
                        [0.7, 0.4, 3.0, 0.5, 2.0, 1.0],             # nothing within 1e-4
                        [0.5, 0.5, 2.0, 1.0, 2.0, 1.0]], dtype=torch.float64)   # a row of no image (B = 1)
    per_match, cells = _detlossref.kink_mask(pi, idx, box)
    assert per_match.tolist() == [True, False]
    assert cells.view(-1).tolist() == [True, False]
    box[0, 2] = 2.0
    box[0, 0] = 0.5 + 2.0 + 5e-5                                    # disjoint in x, l2 = r1 + 5e-5: iwr = -5e-5
    per_match, _ = _detlossref.kink_mask(pi, idx, box)
    k, _ = _detlossref.kink_quantities(pi, idx, box)
    assert abs(float(k[0, 4]) + 5e-5) < 1e-9 and per_match.tolist() == [True, False]
