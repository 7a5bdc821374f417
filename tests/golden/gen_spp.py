#!/usr/bin/env python3
"""Golden YOLOv3-SPP: the REFERENCE's own `Model` built from yolov3/models/yolov3-spp.yaml (layer 12 = SPP(512, (5, 9, 13)),
common.py:202-215). Runs only in the build container (the reference never travels to the GPU box).

    python tests/golden/gen_spp.py [--out DIR]

Writes
  yolo_spp.npz                        full width, nc 80, weights `_synth.synth_yolo_state_dict(m, seed=2)`, eval mode:
                                      x [1,3,64,96], pred, raw0..2 (what gen_golden.py's `yolo` records for the plain graph)
  state_dict_keys_spp.json            {"yolo_spp": {state-dict key: shape}} of that model
  yolov3spp_w0625_refpickle.pt        width 0.0625, nc 7, saved the way the reference's trainer saves a checkpoint (a pickled
                                      module of models.yolo.* / models.common.* classes: tensors and class NAMES only)
  yolov3spp_w0625_refpickle_fused.pt  the same module after fuse()
  ckpt_import_spp.npz                 x, pred, raw0 (the unfused module, .float().eval()), pred_fused_fp32, nparams
"""
import contextlib
import copy
import io
import json
import os
import re
import sys
import tempfile

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import matplotlib  # noqa: E402
matplotlib.use("Agg")
import matplotlib.pyplot  # noqa: E402,F401  (before import_reference_yolo: with its IPython stub in place the reference's own
#                                             matplotlib.use('Agg') must find the backend already chosen and pyplot loaded)
import gen_golden  # noqa: E402  (sets MKL_CBWR=COMPATIBLE before numpy loads)

import numpy as np  # noqa: E402
import torch  # noqa: E402
from _synth import synth_yolo_state_dict, test_image  # noqa: E402

YAML = "/root/reference/yolov3/models/yolov3-spp.yaml"


def _build(Model, path, nc):
    with contextlib.redirect_stdout(io.StringIO()), contextlib.redirect_stderr(io.StringIO()):
        return Model(path, ch=3, nc=nc)


def main(out_dir):
    Model = gen_golden.import_reference_yolo()
    m = _build(Model, YAML, 80)
    m.load_state_dict(synth_yolo_state_dict(m, seed=2))
    m.eval()
    x = test_image(1, 64, 96, seed=51, special=False)
    with torch.no_grad():
        pred, raws = m(torch.from_numpy(x))
    out = {"x": x, "pred": pred.numpy()}
    for i, r in enumerate(raws):
        out[f"raw{i}"] = r.numpy()
    np.savez_compressed(os.path.join(out_dir, "yolo_spp.npz"), **out)
    with open(os.path.join(out_dir, "state_dict_keys_spp.json"), "w") as f:
        json.dump({"yolo_spp": {k: list(v.shape) for k, v in m.state_dict().items()}}, f, indent=0)

    text = re.sub(r"width_multiple:\s*[0-9.]+", "width_multiple: 0.0625", open(YAML).read())
    with tempfile.TemporaryDirectory() as tmp:
        ypath = os.path.join(tmp, "yolov3-spp_w0625.yaml")
        open(ypath, "w").write(text)
        m = _build(Model, ypath, 7)
    m.load_state_dict(synth_yolo_state_dict(m, seed=4))
    m.names = {i: f"c{i}" for i in range(7)}
    ckpt = {"epoch": 3, "best_fitness": np.array([0.5]), "model": copy.deepcopy(m).half(), "ema": None, "updates": 0,
            "optimizer": None, "opt": {"weights": "yolov3-spp.pt", "imgsz": 512}, "date": "2025-01-01T00:00:00"}
    path = os.path.join(out_dir, "yolov3spp_w0625_refpickle.pt")
    torch.save(ckpt, path)
    ref = torch.load(path, map_location="cpu", weights_only=False)["model"].float().eval()
    x = test_image(1, 64, 96, seed=52, special=False)
    with torch.no_grad():
        pred, raws = ref(torch.from_numpy(x))
    fused = copy.deepcopy(ref).fuse().eval()
    fpath = os.path.join(out_dir, "yolov3spp_w0625_refpickle_fused.pt")
    torch.save({"model": copy.deepcopy(fused).half()}, fpath)
    fused = torch.load(fpath, map_location="cpu", weights_only=False)["model"].float().eval()
    with torch.no_grad():
        pred_f, _ = fused(torch.from_numpy(x))
    np.savez_compressed(os.path.join(out_dir, "ckpt_import_spp.npz"), x=x, pred=pred.numpy(), raw0=raws[0].numpy(),
                        pred_fused_fp32=pred_f.numpy(), nparams=np.int64(sum(p.numel() for p in ref.parameters())))
    print(f"wrote yolo_spp.npz, state_dict_keys_spp.json, ckpt_import_spp.npz and the two pickles "
          f"({os.path.getsize(path)}, {os.path.getsize(fpath)} bytes) to {out_dir}")


if __name__ == "__main__":
    args = sys.argv[1:]
    if args[:1] == ["--out"]:
        main(args[1])
    elif not args:
        main(HERE)
    else:
        raise SystemExit("usage: gen_spp.py [--out DIR]")
