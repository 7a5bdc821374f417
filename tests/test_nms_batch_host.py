"""adayolo_nms_batch without a device: the argument checks of the C entry (all made before any launch), the ctypes mirror of
its argument block, the workspace function, the errors of the Python layers above it, and the one property of the HOST path
that the kernel has to reproduce and that no other host test pins: thresholds are compared in fp32."""
import ctypes

import numpy as np
import pytest
import torch

P = 0x10000000                                                       # a fake device address: every call fails its checks first


def _args(**over):
    from adaptiveisp_amd.yolo import _lib
    a = _lib.NmsBatchArgs()
    base = dict(pred=P, pred_row_stride=8, B=2, N=10, nc=3, conf_thres=0.25, iou_thres=0.45, max_det=300, max_nms=30000, cap=30,
                flags=0, workspace=P, workspace_bytes=1 << 30, det=P, det_offset=P, status=P)
    for k, v in dict(base, **over).items():
        setattr(a, k, v)
    return a


def test_exports_and_struct_layout():
    from adaptiveisp_amd.yolo import _lib
    L = _lib.load()
    assert {"adayolo_nms_batch", "adayolo_nms_batch_workspace_bytes"} <= set(_lib.EXPORTS)
    assert hasattr(L, "adayolo_nms_batch") and hasattr(L, "adayolo_nms_batch_workspace_bytes")
    # include/adayolo.h on LP64: pointer, 4 x int32, 2 x float, 4 x int32, pointer, size_t, 3 pointers
    A = _lib.NmsBatchArgs
    assert ctypes.sizeof(A) == 88
    assert [getattr(A, f).offset for f, _ in A._fields_] == [0, 8, 12, 16, 20, 24, 28, 32, 36, 40, 44, 48, 56, 64, 72, 80]
    hdr = open(__import__("os").path.join(__import__("os").path.dirname(_lib._HERE), "include", "adayolo.h")).read()
    body = hdr.split("typedef struct adayolo_nms_batch_args {", 1)[1].split("} adayolo_nms_batch_args;", 1)[0]
    import re
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    names = [n.strip() for decl in body.split(";") if decl.strip() for n in decl.strip().split(None, 1)[1].replace("*", " ").split(",")]
    names = [n.split()[-1] for n in names]
    assert names == [f for f, _ in A._fields_]
    assert (_lib.NMS_MULTI_LABEL, _lib.NMS_AGNOSTIC, _lib.NMS_OVERFLOW) == (1, 2, 1)
    for macro, v in (("ADAYOLO_NMS_MULTI_LABEL", 1), ("ADAYOLO_NMS_AGNOSTIC", 2), ("ADAYOLO_NMS_OVERFLOW", 1)):
        assert re.search(rf"#define {macro}\s+{v}\b", hdr)


def test_argument_checks_without_gpu():
    from adaptiveisp_amd.yolo import _lib
    fn = _lib.load().adayolo_nms_batch
    EINVAL, ESHAPE = -1, -2
    assert fn(None, None) == EINVAL
    for ptr in ("pred", "workspace", "det", "det_offset", "status"):
        assert fn(ctypes.byref(_args(**{ptr: None})), None) == EINVAL, ptr
    bad = dict(nc=[0, -1], conf_thres=[-0.01, 1.01, float("nan")], iou_thres=[-0.01, 1.01, float("nan")], max_det=[0, -3],
               max_nms=[0, -1], cap=[0, -1], flags=[4, 8, 7, -1], workspace_bytes=[0, 100])
    for k, values in bad.items():
        for v in values:
            assert fn(ctypes.byref(_args(**{k: v})), None) == ESHAPE, (k, v)
    assert fn(ctypes.byref(_args(N=1 << 29, nc=4, pred_row_stride=9)), None) == ESHAPE          # N*nc = 2^31
    assert fn(ctypes.byref(_args(N=(1 << 29) - 1, nc=4, pred_row_stride=9, B=1, workspace_bytes=0)), None) == ESHAPE  # fits; no workspace
    assert fn(ctypes.byref(_args(pred_row_stride=7)), None) == ESHAPE                            # rows overlap: 5 + nc = 8
    # the thresholds' closed ends are fine, and an empty problem is no launch: 0 with fake addresses and no device
    need = _lib.load().adayolo_nms_batch_workspace_bytes(0, 10, 3, 30, 30000, 300)
    for kw in (dict(B=0), dict(N=0), dict(B=0, conf_thres=0.0, iou_thres=1.0), dict(N=0, conf_thres=1.0, iou_thres=0.0)):
        assert fn(ctypes.byref(_args(**kw)), None) == 0, kw
    assert fn(ctypes.byref(_args(B=0, workspace_bytes=need)), None) == 0
    # a workspace one byte short is refused, also for the empty problem's (the check comes first)
    need = _lib.load().adayolo_nms_batch_workspace_bytes(2, 0, 3, 30, 30000, 300)
    assert fn(ctypes.byref(_args(N=0, workspace_bytes=need - 1)), None) == ESHAPE
    assert fn(ctypes.byref(_args(N=0, workspace_bytes=need)), None) == 0


def test_workspace_bytes_non_decreasing_and_linear():
    from adaptiveisp_amd.yolo import _lib
    ws = _lib.load().adayolo_nms_batch_workspace_bytes
    base = dict(B=4, N=1000, nc=3, cap=3000, max_nms=30000, max_det=300)
    order = list(base)
    steps = dict(B=[1, 2, 3, 4, 5, 8, 64], N=[1, 10, 1000, 100000], nc=[1, 3, 80], cap=[1, 2, 63, 64, 65, 3000, 4096, 4097, 131072],
                 max_nms=[1, 100, 30000, 1 << 20], max_det=[1, 5, 300, 2048])
    for k, values in steps.items():
        got = [ws(*[dict(base, **{k: v})[name] for name in order]) for v in values]
        assert all(g > 0 for g in got) and got == sorted(got), (k, got)
    # linear in B * cap: 8 bytes per slot with cap rounded up to a power of two, plus the staged rows
    assert ws(8, 1000, 3, 131072, 30000, 300) <= 8 * 131072 * 8 + 8 * 300 * 24 + 1024
    assert ws(8, 1000, 3, 100000, 30000, 300) <= 2 * (8 * 100000 * 8) + 8 * 300 * 24 + 1024
    assert ws(2, 1, 1, 1, 1, 1) < 2048


def test_python_layers_refuse_what_cannot_run():
    from _engine import cpu_agent
    from adaptiveisp_amd.config import cfg
    from adaptiveisp_amd.val import non_max_suppression_device, run_eval
    from adaptiveisp_amd.yolo import _lib
    agent = cpu_agent(cfg)
    with pytest.raises(ValueError, match="HIP device"):
        run_eval(agent, lambda x: x, [], cfg, match="device", nms="device")
    with pytest.raises(ValueError, match="HIP device"):
        run_eval(agent, lambda x: x, [], cfg, nms="device")
    with pytest.raises(ValueError, match="bogus"):
        run_eval(agent, lambda x: x, [], cfg, nms="bogus")
    pred = torch.zeros(1, 4, 8)
    with pytest.raises(_lib.AdayoloError, match="device"):
        non_max_suppression_device(pred, 0.25, 0.45)
    with pytest.raises(_lib.AdayoloError, match="device"):
        _lib.nms_batch(pred, 0.25, 0.45, 300, 30000, 12, True, False)
    with pytest.raises(ValueError):
        non_max_suppression_device(pred, 1.5, 0.45)


class _OnDevice(torch.nn.Module):
    """An agent that claims to live on a HIP device without one being touched: run_eval's argument checks read no more than
    the device of its first parameter."""

    def __init__(self):
        super().__init__()
        self.filters = []

    def parameters(self, recurse=True):
        class _P:
            device = torch.device("cuda", 0)
        return iter([_P()])


def test_run_eval_argument_combinations():
    from adaptiveisp_amd.config import cfg
    from adaptiveisp_amd.val import run_eval
    agent = _OnDevice()
    with pytest.raises(ValueError, match="match='device'"):
        run_eval(agent, lambda x: x, [], cfg, nms="device")                                   # match stays "host"
    with pytest.raises(ValueError, match="nms_fn"):
        run_eval(agent, lambda x: x, [], cfg, match="device", nms="device", nms_fn=lambda b, s, t: None)
    with pytest.raises(ValueError, match="bogus"):
        run_eval(agent, lambda x: x, [], cfg, match="device", nms="bogus")


def test_cli_flag_parses_and_implies_device_matching(capsys):
    from adaptiveisp_amd.val.__main__ import build_parser
    ap = build_parser()
    base = ["--isp-ckpt", "a", "--detector-ckpt", "b", "--data", "c"]
    assert ap.parse_args(base).nms == "host"
    assert ap.parse_args(base + ["--nms", "device"]).nms == "device"
    with pytest.raises(SystemExit):
        ap.parse_args(base + ["--nms", "elsewhere"])


def test_host_path_compares_thresholds_in_fp32(oracle_mod):
    """conf_thres is a Python double, the scores are fp32: the host path's `>` happens in fp32, i.e. against float32(conf). A
    score EQUAL to float32(conf) is no candidate although it is above the double 0.001 (float32(0.001) > 0.001), the next float
    up is one. The kernel takes conf_thres as a C float, so it sees float32(conf): the same comparison."""
    from adaptiveisp_amd.val import non_max_suppression

    def oracle(boxes, scores, thr):
        order = torch.argsort(scores, descending=True, stable=True)
        return order[torch.from_numpy(oracle_mod.nms(boxes[order].numpy(), thr, max_det=max(boxes.shape[0], 1)))]

    for conf in (0.001, 0.25, 0.1):
        c32 = np.float32(conf)
        up, down = np.nextafter(c32, np.float32(2)), np.nextafter(c32, np.float32(-1))
        for multi in (False, True):
            for where in ("obj", "product"):
                kept = []
                for v in (down, c32, up):
                    pred = torch.zeros(1, 1, 7)
                    pred[0, 0, :4] = torch.tensor([50.0, 50.0, 10.0, 10.0])
                    # the value under test as the objectness (class score 1 -> the product is the same float), or as the
                    # product alone with an objectness of 1
                    pred[0, 0, 4] = float(v) if where == "obj" else 1.0
                    pred[0, 0, 5] = 1.0 if where == "obj" else float(v)
                    out = non_max_suppression(pred, conf, 0.5, multi_label=multi, nms_fn=oracle)
                    kept.append(out[0].shape[0])
                assert kept == [0, 0, 1], (conf, multi, where, kept, float(c32) > conf)
