"""YOLOv3-SPP on the device: adayolo_spp_fwd / adayolo_spp_bwd against the float64 restatement (tests/_sppref.py), the SPP
detector through the inference engine, the checkpoint importer and the training engine (gradient to the image, graph replay),
and both command lines."""
import ctypes
import functools
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import _margins
import _sppref
from _margins import close, close_scaled

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden")

# B, H, W, C: every map size from one pixel over "every window is the whole map" (<= 7 x 7), a 13-window that is partial
# (13 x 14, 16 x 16), more than one 16 x 16 tile in each direction with ragged edges (23 x 40, 33 x 47) — and C from one lane per
# pixel over odd group counts (3, 9) to the production 512
CASES = [(1, 1, 1, 8), (3, 2, 3, 24), (1, 5, 5, 512), (3, 6, 7, 72), (1, 7, 13, 72), (1, 13, 14, 512), (3, 16, 16, 24),
         (1, 23, 40, 32), (1, 33, 47, 24), (3, 33, 47, 8)]


def _p(t):
    return ctypes.c_void_p(t.data_ptr())


def _bf16(a):
    return torch.from_numpy(np.asarray(a, np.float32)).to(torch.bfloat16)


@functools.lru_cache(maxsize=None)
def _case(case, kind):
    """(x, grad_out) bf16 on the host and the float64 reference (forward, grad_x, S) of one case: computed once, shared."""
    B, H, W, C = case
    rng = np.random.default_rng([B, H, W, C, ("random", "ties", "constant").index(kind)])
    if kind == "random":
        x = rng.standard_normal((B, H, W, C))
    elif kind == "ties":
        x = rng.integers(0, 4, (B, H, W, C)).astype(np.float64) - 1.5
    else:
        x = np.full((B, H, W, C), -0.375)
    x, go = _bf16(x), _bf16(rng.standard_normal((B, H, W, 3 * C)))
    xd, god = x.double().numpy(), go.double().numpy()
    gx, S = _sppref.backward(xd, god)
    return x, go, _sppref.forward(xd), gx, S


def _spp_fwd(x, out):
    from adaptiveisp_amd.yolo import _lib
    B, H, W, C = x.shape
    _lib.check(_lib.load().adayolo_spp_fwd(_p(x), x.stride(2), _p(out), out.stride(2), B, H, W, C, _lib.stream_ptr()), "spp_fwd")
    torch.cuda.synchronize()


def _spp_bwd(x, go, gx, accumulate):
    from adaptiveisp_amd.yolo import _lib
    B, H, W, C = x.shape
    _lib.check(_lib.load().adayolo_spp_bwd(_p(x), x.stride(2), _p(go), go.stride(2), _p(gx), gx.stride(2), int(accumulate), B, H, W,
                                           C, _lib.stream_ptr()), "spp_bwd")
    torch.cuda.synchronize()


@pytest.mark.parametrize("case", CASES)
def test_spp_forward_kernel_equals_float64(case):
    B, H, W, C = case
    x, _, ref, _, _ = _case(case, "random")
    ref = torch.from_numpy(ref).float()
    # the production layout: x is channel slice 0 and out slices 1..3 of one [B,H,W,4C] tensor
    cat = torch.full((B, H, W, 4 * C), 7.0, dtype=torch.bfloat16, device=DEV)
    cat[..., :C] = x.to(DEV)
    _spp_fwd(cat[..., :C], cat[..., C:])
    assert torch.equal(cat[..., C:].float().cpu(), ref) and torch.equal(cat[..., :C].cpu(), x)
    # separate tensors inside wider ones: padded strides, sentinels outside every written range
    xw = torch.full((B, H, W, C + 16), 3.0, dtype=torch.bfloat16, device=DEV)
    ow = torch.full((B, H, W, 3 * C + 24), 5.0, dtype=torch.bfloat16, device=DEV)
    xw[..., 8:8 + C] = x.to(DEV)
    _spp_fwd(xw[..., 8:8 + C], ow[..., 16:16 + 3 * C])
    assert torch.equal(ow[..., 16:16 + 3 * C].float().cpu(), ref)
    assert (ow[..., :16] == 5).all() and (ow[..., 16 + 3 * C:] == 5).all()
    assert (xw[..., :8] == 3).all() and (xw[..., 8 + C:] == 3).all() and torch.equal(xw[..., 8:8 + C].cpu(), x)


@pytest.mark.parametrize("kind", ["random", "ties", "constant"])
@pytest.mark.parametrize("case", CASES)
def test_spp_backward_kernel_vs_float64(case, kind):
    """|got - ref| <= 2^-8 |ref| + 2^-15 S, S = the sum of |contributions| of the element. Derived, not measured: one rounding
    to bf16 costs 2^-9 |ref|, an fp32 sum of at most 276 terms (25 + 81 + 169 windows can name one pixel, + the value already
    there) at most 276 * 2^-24 S < 2^-15 S; each term has 2x slack."""
    B, H, W, C = case
    x, go, _, ref, S = _case(case, kind)
    old = _bf16(np.random.default_rng(11).standard_normal((B, H, W, C)))
    for accumulate in (0, 1):
        # production layout: grad_out is slices 1..3, grad_x slice 0 of one tensor
        G = torch.empty((B, H, W, 4 * C), dtype=torch.bfloat16, device=DEV)
        G[..., :C], G[..., C:] = old.to(DEV), go.to(DEV)
        xd = x.to(DEV)
        _spp_bwd(xd, G[..., C:], G[..., :C], accumulate)
        got = G[..., :C].clone()
        want = ref + (old.double().numpy() if accumulate else 0.0)
        s = S + (np.abs(old.double().numpy()) if accumulate else 0.0)
        err = np.abs(got.double().cpu().numpy() - want)
        bound = 2.0 ** -8 * np.abs(want) + 2.0 ** -15 * s
        worst = float((err / np.maximum(bound, 1e-300)).max()) if (err > 0).any() else 0.0
        print(f"spp_bwd {case} {kind} accumulate={accumulate}: max err {err.max():.3e}, worst share of the bound {worst:.3f}")
        assert (err <= bound).all(), (case, kind, accumulate, float(err.max()), worst)
        assert torch.equal(G[..., C:].cpu(), go)                                     # grad_out untouched
        # a second run from the same state: the same bits
        G2 = torch.empty_like(G)
        G2[..., :C], G2[..., C:] = old.to(DEV), go.to(DEV)
        _spp_bwd(xd, G2[..., C:], G2[..., :C], accumulate)
        assert torch.equal(G2[..., :C].view(torch.int16), got.view(torch.int16))
    # separate tensors with padded strides: nothing outside grad_x's channels is written
    xw = torch.full((B, H, W, C + 8), 2.0, dtype=torch.bfloat16, device=DEV)
    gw = torch.full((B, H, W, C + 24), 9.0, dtype=torch.bfloat16, device=DEV)
    gow = torch.full((B, H, W, 3 * C + 8), 4.0, dtype=torch.bfloat16, device=DEV)
    xw[..., :C], gow[..., 8:] = x.to(DEV), go.to(DEV)
    _spp_bwd(xw[..., :C], gow[..., 8:], gw[..., 16:16 + C], 0)
    err = np.abs(gw[..., 16:16 + C].double().cpu().numpy() - ref)
    assert (err <= 2.0 ** -8 * np.abs(ref) + 2.0 ** -15 * S).all()
    assert (gw[..., :16] == 9).all() and (gw[..., 16 + C:] == 9).all() and (gow[..., :8] == 4).all()


def _spp_model():
    from _synth import synth_yolo_state_dict
    from adaptiveisp_amd.yolo import yolov3_spp
    m = yolov3_spp().eval()
    m.load_state_dict(synth_yolo_state_dict(m))
    return m


@pytest.mark.parametrize("shape,tune", [((1, 64, 96), False), ((2, 224, 256), False), ((1, 64, 96), True)])
def test_spp_engine_vs_reference_model(golden, shape, tune):
    from _synth import test_image
    from adaptiveisp_amd.yolo import YoloEngine
    B, H, W = shape
    m = _spp_model()
    x = torch.from_numpy(golden("yolo_spp")["x"] if shape == (1, 64, 96) else test_image(B, H, W, seed=77, special=False))
    eng = YoloEngine(m, B, H, W, device=DEV)
    kinds = [k for k, _, _ in eng.plan]
    assert kinds.count("spp") == 1 and [o["kind"] for o in eng.ops].count("spp") == 1
    i = kinds.index("spp")
    assert kinds[i - 1] == kinds[i + 1] == "conv" and eng.plan[i + 1][2][11] == 2048 and eng.plan[i + 1][2][12] == 512
    if tune:
        entry = eng.plan[i]
        eng.autotune(cache=None, write=False)
        assert [e for e in eng.plan if e[0] == "spp"] == [entry]                      # every plan rewrite passes it through
    seen = []
    eng.hook = seen.append
    pred = eng(x.to(DEV))
    eng.hook = None
    if eng.fuse_head:
        assert seen == list(range(eng.num_launches()))                                # the pool is one launch of the forward
    torch.cuda.synchronize()
    boxed = torch.full((B, 3, eng.Hp, W), 114 / 255)
    boxed[:, :, eng.pad_top:eng.pad_top + H] = x
    with torch.no_grad():
        ref_pred, ref_raw = m(boxed)
    if shape == (1, 64, 96):
        np.testing.assert_allclose(ref_pred.numpy(), golden("yolo_spp")["pred"], rtol=1e-5, atol=1e-6)   # the reference itself
    for r, rr in zip(eng.raw_maps(), ref_raw):
        close_scaled("yolo.spp_engine_raw_maps_vs_fp32_module_tree", r.cpu(), rr, 3e-2, floor=0.0,
                     err_msg="raw head maps (bf16 SPP engine vs fp32 reference)")
    close("yolo.spp_engine_pred_vs_fp32_module_tree", pred.cpu(), ref_pred, rtol=2e-2, atol=2e-2)


@pytest.mark.parametrize("fused", [False, True])
def test_imported_spp_pickle_through_the_hip_engine(golden, fused):
    from adaptiveisp_amd.yolo import YoloEngine
    from adaptiveisp_amd.yolo.checkpoint import load_detector_checkpoint
    g = golden("ckpt_import_spp")
    name = "yolov3spp_w0625_refpickle_fused.pt" if fused else "yolov3spp_w0625_refpickle.pt"
    m = load_detector_checkpoint(os.path.join(GOLD, name)).eval()
    x = torch.from_numpy(g["x"])
    B, _, H, W = x.shape
    eng = YoloEngine(m, B, H, W, device=DEV)
    assert eng._stem is None and eng.plan[0][0] == "pack" and sum(1 for e in eng.plan if e[0] == "spp") == 1
    pred = eng(x.to(DEV)).cpu().numpy()
    ref = g["pred_fused_fp32"] if fused else g["pred"]
    rel = np.abs(pred - ref) / (np.abs(ref) + 1.0)
    assert rel.max() < 2e-2, rel.max()
    raw0 = eng.raw_maps()[0].cpu().numpy()
    if not fused:
        assert np.abs(raw0 - g["raw0"]).max() <= 3e-2 * np.abs(g["raw0"]).max()
    conf = ref[..., 4] * ref[..., 5:].max(-1)
    top = np.argsort(-conf[0])[:20]
    np.testing.assert_allclose(pred[0, top, :4], ref[0, top, :4], rtol=3e-2, atol=0.5)


def _frozen_spp():
    det = _spp_model().to(DEV).train()
    for m in det.modules():
        if isinstance(m, torch.nn.BatchNorm2d):
            m.eval()
    for p in det.parameters():
        p.requires_grad_(False)
    return det


# P5 maps: 2 x 3 (every window is the whole map), 7 x 8, 14 x 15 (a 13-window is partial)
@pytest.mark.parametrize("B,H,W", [(2, 64, 96), (1, 224, 256), (1, 448, 480)])
def test_spp_backward_to_image_vs_fp32_autograd(B, H, W):
    """The SPP detector's image gradient on the HIP training engine against fp32 autograd of the module tree, held to what an
    independent bf16 run of the same network (torch autocast) loses, with the project's margin of 1.25."""
    from _synth import test_image
    from adaptiveisp_amd.yolo import YoloTrainEngine
    det = _frozen_spp()
    eng = YoloTrainEngine(det, B, H, W, device=DEV)
    assert [e[0] for e in eng.tfwd].count("spp") == 1 and [e[0] for e in eng.tbwd].count("sppbwd") == 1
    x = torch.from_numpy(test_image(B, H, W, seed=61, special=False)).to(DEV)
    Hp = (H + 31) // 32 * 32
    top = (Hp - H) // 2
    g = torch.Generator().manual_seed(5)
    xr = x.clone().requires_grad_(True)
    boxed = torch.full((B, 3, Hp, W), 114.0 / 255.0, device=DEV)
    boxed = torch.cat([boxed[:, :, :top], xr, boxed[:, :, top + H:]], 2) if Hp != H else xr
    raws_ref = det(boxed)
    R = [torch.randn(r.shape, generator=g).to(DEV) for r in raws_ref]
    sum((r * w).sum() for r, w in zip(raws_ref, R)).backward()
    xh = x.clone().requires_grad_(True)
    raws = eng(xh)
    for a, b in zip(raws, raws_ref):
        assert (a - b.detach()).abs().max() <= 5e-2 * max(1.0, b.abs().max().item())
    sum((r * w).sum() for r, w in zip(raws, R)).backward()
    torch.cuda.synchronize()
    gh, gr = xh.grad, xr.grad
    assert torch.isfinite(gh).all()
    rel = ((gh - gr).norm() / gr.norm()).item()
    cos = F.cosine_similarity(gh.reshape(1, -1), gr.reshape(1, -1)).item()
    xa = x.clone().requires_grad_(True)
    boxed_a = torch.cat([boxed.detach()[:, :, :top], xa, boxed.detach()[:, :, top + H:]], 2) if Hp != H else xa
    with torch.autocast("cuda", dtype=torch.bfloat16):
        raws_a = det(boxed_a)
    sum((r.float() * w).sum() for r, w in zip(raws_a, R)).backward()
    rel_a = ((xa.grad - gr).norm() / gr.norm()).item()
    cos_a = F.cosine_similarity(xa.grad.reshape(1, -1), gr.reshape(1, -1)).item()
    msg = (f"SPP detector image gradient vs fp32 autograd at {B}x{H}x{W}: HIP engine rel {rel:.4f} cos {cos:.6f} | "
           f"torch autocast-bf16 rel {rel_a:.4f} cos {cos_a:.6f}")
    print(msg)
    _margins.NOTES.append(msg)
    assert rel <= 1.25 * rel_a, (rel, rel_a)
    assert 1.0 - cos <= 1.25 ** 2 * (1.0 - cos_a), (cos, cos_a)
    # the project's caps for the plain detector hold too — unless the independent bf16 run itself misses them
    if rel_a < 0.025 and cos_a > 0.9995:
        assert rel < 0.025 and cos > 0.9995, (rel, cos)


def test_spp_graph_replay_changes_nothing():
    """The SPP training engine with its launch sequences replayed from hipGraphs, conv + SiLU pairs fused and SiLU' absorbed,
    against the same engine with all three switched off: raw head maps and image gradient bit for bit, replay after replay."""
    from _synth import test_image
    from adaptiveisp_amd.yolo import YoloTrainEngine
    det = _frozen_spp()
    B, H, W = 2, 224, 256
    x = torch.from_numpy(test_image(B, H, W, seed=5, special=False)).to(DEV)
    results = []
    for on in ("0", "1"):
        for k in ("ADAYOLO_TRAIN_GRAPH", "ADAYOLO_TRAIN_KEEP", "ADAYOLO_TRAIN_FUSE_DSILU"):
            os.environ[k] = on
        try:
            eng = YoloTrainEngine(det, B, H, W, device=DEV)
            outs = []
            for rep in range(2):                                        # second pass = a replay when graphs are on
                xr = x.clone().requires_grad_(True)
                raws = eng(xr)
                if rep == 0:
                    R = [torch.randn(r.shape, generator=torch.Generator().manual_seed(3 + i)).to(DEV) for i, r in enumerate(raws)]
                sum((r * w).sum() for r, w in zip(raws, R)).backward()
                torch.cuda.synchronize()
                outs.append(([r.detach().clone() for r in raws], xr.grad.clone()))
            assert all(torch.equal(a, b) for a, b in zip(outs[0][0], outs[1][0])) and torch.equal(outs[0][1], outs[1][1])
            if on == "1":
                assert eng._graphs["fwd"] is not None and eng._graphs["bwd"] is not None
                assert sum(1 for e in eng._backward_plan() if e[0] == "sppbwd") == 1
            results.append(outs[1])
        finally:
            for k in ("ADAYOLO_TRAIN_GRAPH", "ADAYOLO_TRAIN_KEEP", "ADAYOLO_TRAIN_FUSE_DSILU"):
                os.environ.pop(k, None)
    (raw_a, grad_a), (raw_b, grad_b) = results
    assert all(torch.equal(a, b) for a, b in zip(raw_a, raw_b)) and torch.equal(grad_a, grad_b)
    assert grad_a.abs().max() > 0


# ---------------------------------------------------------------------------------------------------------- command lines
def test_val_cli_with_the_spp_pickle(tmp_path):
    from PIL import Image
    from _synth import synth_state_dict
    from adaptiveisp_amd.agent import Agent
    from adaptiveisp_amd.config import cfg
    os.makedirs(tmp_path / "data" / "images")
    os.makedirs(tmp_path / "data" / "labels")
    rng = np.random.default_rng(3)
    for i, (h, w) in enumerate([(80, 96), (64, 64), (70, 50)]):
        Image.fromarray((rng.random((h, w, 3)) * 120).astype(np.uint8)).save(tmp_path / "data" / "images" / f"im{i}.png")
        np.savetxt(tmp_path / "data" / "labels" / f"im{i}.txt", [[i % 7, 0.5, 0.5, 0.3, 0.4]], fmt="%.6f")
    agent = Agent(cfg, shape=(6 + len(cfg.filters), 64, 64))
    torch.save({"iter": 0, "agent_model": synth_state_dict(agent, seed=0)}, tmp_path / "agent.pth")
    cmd = ["timeout", "-k", "10", "600", sys.executable, "-m", "adaptiveisp_amd.val", "--isp-ckpt", str(tmp_path / "agent.pth"),
           "--detector-ckpt", os.path.join(GOLD, "yolov3spp_w0625_refpickle.pt"), "--data", str(tmp_path / "data" / "images"),
           "--img-size", "64", "--batch-size", "2", "--project", str(tmp_path / "runs"), "--name", "spp"]
    env = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
    r = subprocess.run(cmd, cwd=ROOT, env=env, capture_output=True, text=True)
    assert r.returncode == 0, f"exit {r.returncode}\n{r.stdout[-3000:]}\n{r.stderr[-3000:]}"
    assert "mAP50-95" in r.stdout and "Results saved to" in r.stdout
    run = r.stdout.strip().splitlines()[-1].split("Results saved to ", 1)[1]
    res = json.load(open(os.path.join(run, "results.json")))
    assert all(np.isfinite(res[k]) for k in ("mp", "mr", "map50", "map"))
    # a --detector-cfg that contradicts the file is a usage error that names both, before any device work
    r = subprocess.run(cmd + ["--detector-cfg", "yolov3"], cwd=ROOT, env=env, capture_output=True, text=True)
    assert r.returncode == 2 and "--detector-cfg yolov3 " in r.stderr and "a yolov3-spp graph" in r.stderr


def test_train_cli_with_the_spp_detector():
    cache = os.path.join(ROOT, "adaptiveisp_amd", "yolo", "tuning", "mi355x.json")
    saved = open(cache, "rb").read()              # the CLI autotunes into the committed table: give it back as it was
    try:
        r = subprocess.run(["timeout", "-k", "10", "600", sys.executable, "-m", "adaptiveisp_amd.train", "--detector-cfg",
                            "yolov3-spp", "--iters", "2", "--batch", "2", "--size", "64"], cwd=ROOT, capture_output=True, text=True)
    finally:
        with open(cache, "wb") as f:
            f.write(saved)
    assert r.returncode == 0, r.stderr[-3000:]
    line = json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("{")][-1])
    last = line["last"]
    assert np.isfinite([last["agent_loss"], last["value_loss"], last["reward"]]).all(), last
