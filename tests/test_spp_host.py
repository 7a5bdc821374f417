"""YOLOv3-SPP without a GPU: the float64 restatement of the pyramid pooling against torch-CPU (forward and the routing of the
gradient, ties included), the module tree against the reference's own SPP model (golden vectors of tests/golden/gen_spp.py),
the checkpoint importer on the reference's SPP pickles, the C-ABI's refusals and the command lines' --detector-cfg."""
import ctypes
import json
import os
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import _sppref

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
SPP_PT = os.path.join(GOLD, "yolov3spp_w0625_refpickle.pt")
SPP_FUSED_PT = os.path.join(GOLD, "yolov3spp_w0625_refpickle_fused.pt")
PLAIN_PT = os.path.join(GOLD, "yolov3_w0625_refpickle.pt")


def _inputs(kind, B, H, W, C, seed):
    rng = np.random.default_rng(seed)
    if kind == "random":
        return rng.standard_normal((B, H, W, C))
    if kind == "ties":                                        # four values: almost every window has several maxima
        return rng.integers(0, 4, (B, H, W, C)).astype(np.float64) - 1.5
    return np.full((B, H, W, C), 0.75)


@pytest.mark.parametrize("kind", ["random", "ties", "constant"])
@pytest.mark.parametrize("H,W", [(2, 3), (7, 9), (13, 14)])
def test_sppref_equals_torch_max_pool_and_its_autograd(kind, H, W):
    B, C = 2, 3
    x = _inputs(kind, B, H, W, C, seed=H * 100 + W)
    go = np.random.default_rng(7).standard_normal((B, H, W, 3 * C))
    xt = torch.from_numpy(x).permute(0, 3, 1, 2).contiguous().requires_grad_(True)
    pools = [F.max_pool2d(xt, k, 1, k // 2) for k in _sppref.KS]
    ref = torch.cat(pools, 1)
    assert np.array_equal(_sppref.forward(x), ref.detach().permute(0, 2, 3, 1).numpy())
    ref.backward(torch.from_numpy(go).permute(0, 3, 1, 2).contiguous())
    gx, S = _sppref.backward(x, go)
    np.testing.assert_allclose(gx, xt.grad.permute(0, 2, 3, 1).numpy(), rtol=0, atol=1e-12 * max(1.0, S.max()))
    assert S.shape == gx.shape and (S >= np.abs(gx) - 1e-12).all()
    assert abs(S.sum() - np.abs(go).sum()) <= 1e-9 * np.abs(go).sum()      # every contribution lands somewhere, once
    # the identity the forward kernel is built on: clipped 9- and 13-pools are cascaded 5-pools
    mp5 = lambda t: F.max_pool2d(t, 5, 1, 2)                                # noqa: E731
    assert torch.equal(mp5(mp5(xt)), pools[1]) and torch.equal(mp5(mp5(mp5(xt))), pools[2])


def test_spp_state_dict_layout_matches_reference():
    from adaptiveisp_amd.yolo import yolov3, yolov3_spp
    ref = json.load(open(os.path.join(GOLD, "state_dict_keys_spp.json")))["yolo_spp"]
    m = yolov3_spp()
    assert {k: list(v.shape) for k, v in m.state_dict().items()} == ref
    assert list(m.state_dict()["model.12.cv2.conv.weight"].shape) == [512, 2048, 1, 1]
    assert len(m.model) == 29 and m.model[-1].f == (27, 22, 15) and not list(m.model[12].m.parameters())
    # the default stays plain YOLOv3 with its own key layout
    plain = json.load(open(os.path.join(GOLD, "state_dict_keys.json")))["yolo"]
    assert {k: list(v.shape) for k, v in yolov3().state_dict().items()} == plain


def test_spp_torch_forward_matches_reference(golden):
    from _synth import synth_yolo_state_dict
    from adaptiveisp_amd.yolo import yolov3_spp
    g = golden("yolo_spp")
    m = yolov3_spp().eval()
    m.load_state_dict(synth_yolo_state_dict(m))
    with torch.no_grad():
        pred, raws = m(torch.from_numpy(g["x"]))
    np.testing.assert_allclose(pred.numpy(), g["pred"], rtol=1e-5, atol=1e-6)
    for i, r in enumerate(raws):
        np.testing.assert_allclose(r.numpy(), g[f"raw{i}"], rtol=1e-5, atol=1e-6)


def test_cfg_names():
    from adaptiveisp_amd.yolo.model import SPP, Conv, DetectionModel
    for cfg, spp in (("yolov3", False), ("yolov3.yaml", False), ("models/yolov3.yaml", False), ("yolov3-spp", True),
                     ("yolov3-spp.yaml", True), ("/some/where/yolov3-spp.yaml", True)):
        m = DetectionModel(cfg=cfg, nc=3, width=0.0625)
        assert isinstance(m.model[12], SPP if spp else Conv), cfg
        assert m.cfg == ("yolov3-spp" if spp else "yolov3")
    spp = DetectionModel(cfg="yolov3-spp", nc=3, width=0.0625).model[12]
    assert spp.cv1.conv.in_channels == 64 and spp.cv1.conv.out_channels == 32 and spp.cv2.conv.in_channels == 128
    assert [(p.kernel_size, p.stride, p.padding) for p in spp.m] == [(5, 1, 2), (9, 1, 4), (13, 1, 6)]
    for bad in ("yolov5s", "yolov3-tiny.yaml", "", "yolov3-spp.yml"):
        with pytest.raises(ValueError):
            DetectionModel(cfg=bad)


def test_spp_pickles_load_without_reference(golden):
    from adaptiveisp_amd.yolo.checkpoint import load_detector_checkpoint, read_detector_pickle
    from adaptiveisp_amd.yolo.model import SPP, Conv
    assert "models" not in sys.modules and "models.yolo" not in sys.modules
    g = golden("ckpt_import_spp")
    info = read_detector_pickle(SPP_PT)
    assert info["nc"] == 7 and info["source"] == "model" and info["names"] == {i: f"c{i}" for i in range(7)}
    m = load_detector_checkpoint(SPP_PT)
    assert "models" not in sys.modules
    assert m.cfg == "yolov3-spp" and isinstance(m.model[12], SPP)
    assert sum(p.numel() for p in m.parameters()) == int(g["nparams"])
    with torch.no_grad():
        pred, raws = m(torch.from_numpy(g["x"]))
    np.testing.assert_allclose(pred.numpy(), g["pred"], rtol=1e-5, atol=1e-5)
    np.testing.assert_allclose(raws[0].numpy(), g["raw0"], rtol=1e-5, atol=1e-5)
    f = load_detector_checkpoint(SPP_FUSED_PT)
    assert f.cfg == "yolov3-spp"
    with torch.no_grad():
        pred_f, _ = f(torch.from_numpy(g["x"]))
    np.testing.assert_allclose(pred_f.numpy(), g["pred_fused_fp32"], rtol=2e-5, atol=2e-5)
    # the plain pickle still yields the plain graph
    p = load_detector_checkpoint(PLAIN_PT)
    assert p.cfg == "yolov3" and isinstance(p.model[12], Conv)


def test_layout_mismatch_names_both_layouts(monkeypatch):
    from adaptiveisp_amd.yolo import checkpoint
    info = checkpoint.read_detector_pickle(SPP_PT)
    for k in [k for k in info["state_dict"] if k.startswith("model.12.cv2.")]:      # neither layout
        del info["state_dict"][k]
    monkeypatch.setattr(checkpoint, "read_detector_pickle", lambda path: info)
    with pytest.raises(ValueError) as e:
        checkpoint.load_detector_checkpoint(SPP_PT)
    assert "YOLOv3 layout" in str(e.value) and "YOLOv3-SPP layout" in str(e.value) and "model.12.cv2" in str(e.value)


def test_spp_argument_checks_without_gpu():
    """adayolo_spp_fwd / adayolo_spp_bwd refuse before any launch: one case per rule of include/adayolo.h."""
    from adaptiveisp_amd.yolo import _lib
    L = _lib.load()
    assert {"adayolo_spp_fwd", "adayolo_spp_bwd"} <= set(_lib.EXPORTS) and _lib.ABI_VERSION == 10
    EINVAL, ESHAPE = -1, -2
    x, o, g = (ctypes.c_void_p(a) for a in (0x10000000, 0x20000000, 0x30000000))   # never read: every call is refused

    def fwd(x=x, x_cs=64, out=o, out_cs=192, B=2, H=5, W=7, C=64):
        return L.adayolo_spp_fwd(x, x_cs, out, out_cs, B, H, W, C, None)

    def bwd(x=x, x_cs=64, go=o, go_cs=192, gx=g, gx_cs=64, acc=1, B=2, H=5, W=7, C=64):
        return L.adayolo_spp_bwd(x, x_cs, go, go_cs, gx, gx_cs, acc, B, H, W, C, None)

    assert fwd(x=None) == EINVAL and fwd(out=None) == EINVAL
    assert bwd(x=None) == EINVAL and bwd(go=None) == EINVAL and bwd(gx=None) == EINVAL
    for call in (fwd, bwd):
        assert call(C=0) == ESHAPE and call(C=4) == ESHAPE and call(C=-8) == ESHAPE      # C < 8
        assert call(C=12, x_cs=16) == ESHAPE                                             # C % 8
        assert call(x_cs=68) == ESHAPE                                                   # a stride that is no multiple of 8
        assert call(x_cs=56) == ESHAPE                                                   # x_cstride < C
        for dim in ("B", "H", "W"):
            assert call(**{dim: 0}) == ESHAPE and call(**{dim: -1}) == ESHAPE
        assert call(B=4, H=32768, W=32768) == ESHAPE                                     # pixel count beyond 31 bits
        assert call(B=8, H=2048, W=2048) == ESHAPE                                       # 2^25 pixels x 192 channels
    assert fwd(out_cs=196) == ESHAPE and fwd(out_cs=184) == ESHAPE                       # out_cstride % 8, < 3C
    assert bwd(go_cs=196) == ESHAPE and bwd(go_cs=184) == ESHAPE                         # go_cstride % 8, < 3C
    assert bwd(gx_cs=68) == ESHAPE and bwd(gx_cs=56) == ESHAPE                           # gx_cstride % 8, < C
    assert fwd(B=4, H=2048, W=2048, x_cs=64, out_cs=64 * 4) == ESHAPE                    # only out is beyond 31 bits
    assert bwd(B=4, H=2048, W=512, C=256, x_cs=256, go_cs=768, gx_cs=256) == ESHAPE      # only grad_out is


def test_train_cli_detector_cfg(capsys):
    from adaptiveisp_amd.train import build_trainer, parse_args
    import inspect
    assert parse_args([]).detector_cfg == "yolov3"
    assert parse_args(["--detector-cfg", "yolov3-spp"]).detector_cfg == "yolov3-spp"
    assert parse_args(["--detector-ckpt", SPP_PT]).detector_cfg is None                  # the graph comes from the file
    assert parse_args(["--detector-ckpt", SPP_PT, "--detector-cfg", "yolov3-spp"]).detector_cfg == "yolov3-spp"
    with pytest.raises(SystemExit) as e:
        parse_args(["--detector-cfg", "yolov5"])
    assert e.value.code == 2
    capsys.readouterr()
    for ckpt, cfg, have in ((PLAIN_PT, "yolov3-spp", "yolov3"), (SPP_PT, "yolov3", "yolov3-spp")):
        with pytest.raises(SystemExit) as e:
            parse_args(["--detector-ckpt", ckpt, "--detector-cfg", cfg])
        err = capsys.readouterr().err
        assert e.value.code == 2 and f"--detector-cfg {cfg} " in err and f"a {have} graph" in err and ckpt in err
    params = list(inspect.signature(build_trainer).parameters.values())
    assert params[-1].name == "detector_cfg" and params[-1].default == "yolov3"


def test_val_cli_detector_cfg(capsys):
    from adaptiveisp_amd.val.__main__ import parse_args
    base = ["--isp-ckpt", "a", "--data", "c"]
    assert parse_args(base).detector_cfg == "yolov3"
    assert parse_args(base + ["--detector-cfg", "yolov3-spp"]).detector_cfg == "yolov3-spp"
    assert parse_args(base + ["--detector-ckpt", SPP_PT]).detector_cfg is None
    capsys.readouterr()
    with pytest.raises(SystemExit) as e:
        parse_args(base + ["--detector-ckpt", SPP_PT, "--detector-cfg", "yolov3"])
    err = capsys.readouterr().err
    assert e.value.code == 2 and "--detector-cfg yolov3 " in err and "a yolov3-spp graph" in err
