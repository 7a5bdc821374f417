"""Evaluation from the shell — the counterpart of yolov3/val_adaptiveisp.py (`parse_opt` :463-516, `run` :105-460):

    python -m adaptiveisp_amd.val --isp-ckpt ckpt.pth --detector-ckpt yolov3.pt --data lod.yaml --steps 5 --save-image

Images go through data.ImageFolderSource (one pass in file order; `lod`: /255, `coco`: unprocess and noise on the HIP
device), `--batch-size` at a time with the last, partial batch evaluated on a detector engine of its own; the ISP
episode, the detector, NMS, matching and mAP are val.run_eval's. Everything is written under the run directory
(`--project`/`--name`, incremented as exp, exp2, ...): records.txt, results.json, and on request param_results/,
img_results/step-<i>/, labels/<stem>.txt, <detector stem>_predictions.json and confusion_matrix.csv (val/writers.py)."""
import argparse
import json
import math
import os
import time

import numpy as np

HEADER = ("%22s" + "%11s" * 7) % ("Class", "Images", "Instances", "P", "R", "mAP50", "mAP75", "mAP50-95")
ROW = "%22s" + "%11i" * 2 + "%11.3g" * 5


def check_img_size(size, stride=32):
    """`size` rounded up to a multiple of the detector's largest stride (a note is printed when it changes)."""
    new = int(math.ceil(int(size) / stride) * stride)
    if new != int(size):
        print(f"note: --img-size {size} must be a multiple of the max stride {stride}, updating to {new}")
    return new


def increment_path(path, exist_ok=False):
    """runs/val/exp -> runs/val/exp2, exp3, ... while the path exists (unless exist_ok)."""
    path = str(path)
    if not os.path.exists(path) or exist_ok:
        return path
    n = 2
    while os.path.exists(f"{path}{n}"):
        n += 1
    return f"{path}{n}"


def resolve_data(data, task="val"):
    """--data -> (image source for list_images, class names {id: name} or None, nc or None).
    A dataset YAML (`path`, `train` / `val` / `test`, `nc`, `names`, as yolov3/data/lod.yaml): the `task` entry, relative to
    `path`. A relative `path` is taken relative to the YAML's own directory — NOT, as the reference's check_dataset does
    (yolov3/utils/general.py:496-498), relative to the reference's yolov3/ directory: its lod.yaml
    (`path: ../../../datasets/LOD`) therefore names another directory here; give it an absolute `path` or put the YAML
    where the relative one holds. Anything else (a directory, a .txt list, an image) is the source itself."""
    if not (isinstance(data, str) and data.lower().endswith((".yaml", ".yml"))):
        return data, None, None
    import yaml
    with open(data) as f:
        d = yaml.safe_load(f) or {}
    root = str(d.get("path") or "")
    if not os.path.isabs(root):
        root = os.path.normpath(os.path.join(os.path.dirname(os.path.abspath(data)), root))
    if d.get(task) is None:
        raise ValueError(f"{data}: no '{task}' entry")
    entries = d[task] if isinstance(d[task], (list, tuple)) else [d[task]]
    srcs = [e if os.path.isabs(str(e)) else os.path.join(root, str(e)) for e in entries]
    names = d.get("names")
    if isinstance(names, (list, tuple)):
        names = dict(enumerate(names))
    if names is not None:
        names = {int(k): str(v) for k, v in names.items()}
    nc = d.get("nc")
    if nc is None and names is not None:
        nc = len(names)
    if nc is not None and names is not None and int(nc) != len(names):
        raise ValueError(f"{data}: nc = {nc} but {len(names)} names")
    if len(srcs) == 1:
        return srcs[0], names, None if nc is None else int(nc)
    from .loader import list_images
    return [f for s in srcs for f in list_images(s)], names, None if nc is None else int(nc)


def build_parser():
    ap = argparse.ArgumentParser(prog="python -m adaptiveisp_amd.val",
                                 description="Evaluate an ISP policy checkpoint with a YOLOv3 detector (mAP, records, outputs)")
    ap.add_argument("--isp-ckpt", required=True, help="ISP checkpoint (ckpt-*.pth; its 'agent_model' is loaded)")
    ap.add_argument("--detector-ckpt", default=None,
                    help="yolov3.pt or yolov3-spp.pt (default: a random-init detector, for smoke runs only)")
    ap.add_argument("--detector-cfg", default=None, choices=("yolov3", "yolov3-spp"),
                    help="graph of the random-init detector when there is no --detector-ckpt (default: yolov3); a checkpoint "
                         "brings its own graph, and naming the other one is an error")
    ap.add_argument("--data", required=True, help="dataset YAML, or an image directory / .txt list / image")
    ap.add_argument("--task", default="val", choices=("val", "test", "train"), help="which YAML entry to evaluate")
    ap.add_argument("--data-name", default="lod", choices=("lod", "coco", "raw"),
                    help="lod: images / 255; coco: sRGB -> synthetic low-light linear RGB (unprocess_wo_mosaic); raw: real "
                         "captures, one 2-D uint16 .npy colour-filter-array plane per frame at the sensor's size, demosaiced "
                         "(--cfa, --raw-bits, --black-level, --demosaic) and resampled to --img-size in one HIP launch")
    ap.add_argument("--raw-gains", type=float, nargs=3, default=(1.0, 1.0, 1.0), metavar=("R", "G", "B"),
                    help="raw: per-channel multipliers on the demosaiced values (white balance)")
    ap.add_argument("--raw-cal", default=None, metavar="FILE",
                    help="raw: sensor calibration (.npz of python -m adaptiveisp_amd.rawcal): per-position black levels, "
                         "white level, lens shading, defect threshold, applied in one HIP launch before the demosaic")
    ap.add_argument("--raw-dpc", type=int, default=None, metavar="N",
                    help="raw: defect-pixel threshold in sensor counts (overrides the calibration's; alone: defects only)")
    ap.add_argument("--raw-meta", action="store_true",
                    help="raw: read <stem>.json beside each plane: black_level, white_level, gains (as-shot R G B)")
    ap.add_argument("--add-noise", action="store_true", help="coco: shot + read noise")
    ap.add_argument("--bri-range", type=float, nargs=2, default=None, metavar=("LO", "HI"),
                    help="coco: random brightness ratio in [LO, HI)")
    ap.add_argument("--noise-level", type=float, default=None, help="coco: fixed shot noise (default: random)")
    ap.add_argument("--use-linear", action="store_true", help="coco: shot noise uniform instead of log-uniform")
    ap.add_argument("--img-size", type=int, default=512, help="inference size (rounded up to a multiple of 32)")
    ap.add_argument("--batch-size", type=int, default=1)
    ap.add_argument("--steps", type=int, default=5, help="ISP steps per image")
    ap.add_argument("--conf-thres", type=float, default=0.001)
    ap.add_argument("--iou-thres", type=float, default=0.6)
    ap.add_argument("--max-det", type=int, default=300)
    ap.add_argument("--single-cls", action="store_true")
    ap.add_argument("--verbose", action="store_true", help="per-class rows whatever the class count")
    ap.add_argument("--pipeline", default=None, help="forced filter id per step, e.g. 8,3,2,5,7")
    ap.add_argument("--save-param", action="store_true", help="param_results/<stem>.json per batch (--batch-size 1)")
    ap.add_argument("--save-image", action="store_true", help="img_results/step-<i>/<file> after every step")
    ap.add_argument("--save-txt", action="store_true", help="labels/<stem>.txt")
    ap.add_argument("--save-conf", action="store_true", help="confidences in the --save-txt rows")
    ap.add_argument("--save-json", action="store_true", help="COCO-JSON predictions")
    ap.add_argument("--project", default=os.path.join("runs", "val"))
    ap.add_argument("--name", default="exp")
    ap.add_argument("--exist-ok", action="store_true")
    ap.add_argument("--graph", action="store_true", help="replay each batch's ISP episode + detector as one hipGraph")
    ap.add_argument("--match", default="host", choices=("host", "device"),
                    help="where detections are matched to labels: host (torch, per image) or device (one HIP launch per batch)")
    ap.add_argument("--nms", default="host", choices=("host", "device"),
                    help="where NMS runs: host (per image, with a host read each) or device (adayolo_nms_batch: the whole batch "
                         "in four launches, rows left on the device for the matching); device implies --match device")
    ap.add_argument("--confusion", action="store_true",
                    help="confusion_matrix.csv (conf 0.25, IoU 0.45); with --verbose also its per-class counts")
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--tune-cache", default=None, help="detector engine autotune cache (JSON)")
    ap.add_argument("--workers", type=int, default=4, help="decoding threads")
    ap.add_argument("--resize", default="host", choices=("host", "device"),
                    help="where images are resampled to --img-size: host (numpy, in the decoding threads) or device "
                         "(a HIP kernel; use it for photo-sized datasets, where the host resample cannot keep up)")
    ap.add_argument("--sensor", default="rgb", choices=("rgb", "bayer"),
                    help="rgb: the converted image as it is; bayer: through a simulated Bayer sensor (one colour per pixel, "
                         "noise on that sample, quantised) and its demosaic (--demosaic), both HIP kernels")
    ap.add_argument("--demosaic", default="bilinear", choices=("bilinear", "mhc"),
                    help="bayer: 3 x 3 bilinear interpolation, or mhc, the 5 x 5 gradient-corrected one (Malvar-He-Cutler)")
    ap.add_argument("--cfa", default="RGGB", choices=("RGGB", "GRBG", "GBRG", "BGGR"), help="bayer: colour filter array")
    ap.add_argument("--raw-bits", type=int, default=12, help="bayer: sample depth (white level 2^bits - 1)")
    ap.add_argument("--black-level", type=int, default=None, help="bayer: black level (default 2^(bits - 6))")
    return ap


def parse_args(argv=None):
    """Parsed and checked arguments; a usage error exits with status 2 before anything touches a device."""
    from ..config import cfg
    ap = build_parser()
    a = ap.parse_args(argv)
    if a.batch_size < 1 or a.steps < 1:
        ap.error("--batch-size and --steps must be positive")
    try:
        from ..yolo.checkpoint import resolve_detector_cfg
        a.detector_cfg = resolve_detector_cfg(a.detector_ckpt, a.detector_cfg)
    except ValueError as e:
        ap.error(str(e))
    if a.nms == "device" and a.match != "device":
        # the device NMS leaves its rows where adayolo_match reads them: there is no host matching behind it
        print("--nms device: matching runs on the device too (--match device)")
        a.match = "device"
    if a.pipeline is not None:
        try:
            a.pipeline = [int(x) for x in a.pipeline.split(",")]
        except ValueError:
            ap.error(f"--pipeline {a.pipeline!r}: expected comma-separated filter ids")
        if len(a.pipeline) < a.steps:
            ap.error(f"--pipeline has {len(a.pipeline)} ids, fewer than --steps {a.steps}")
        bad = [k for k in a.pipeline if not 0 <= k < len(cfg.filters)]
        if bad:
            ap.error(f"--pipeline ids {bad} outside [0, {len(cfg.filters)})")
    if a.save_param and a.batch_size != 1:
        ap.error(f"--save-param needs --batch-size 1 (got {a.batch_size})")
    if a.data_name == "raw" and a.sensor == "bayer":
        ap.error("--data-name raw with --sensor bayer: the planes already are a sensor's")
    if a.data_name != "raw" and (a.raw_cal is not None or a.raw_dpc is not None or a.raw_meta):
        ap.error("--raw-cal / --raw-dpc / --raw-meta need --data-name raw")
    if a.raw_dpc is not None and a.raw_dpc < 0:
        ap.error(f"--raw-dpc must be >= 0 (got {a.raw_dpc})")
    if a.data_name in ("lod", "raw") and (a.add_noise or a.bri_range is not None):
        print(f"note: --data-name {a.data_name} evaluates the images as they are: --add-noise / --bri-range ignored")
    if a.data_name in ("lod", "raw"):
        a.add_noise, a.bri_range = False, None
    a.img_size = check_img_size(a.img_size)
    if a.graph and (a.save_image or a.save_param):
        print("note: --graph ignored: --save-image / --save-param need the per-step results of the eager loop")
        a.graph = False
    return a


def _batches(source, n_files, batch_size, single_cls=False):
    """One pass over the source in file order: (images [b,3,S,S], targets [n,6], paths, shapes) per batch, the last
    one partial. `single_cls`: every label is class 0, as the reference's dataset makes them (dataloaders.py:549-550)."""
    import torch
    done = 0
    while done < n_files:
        b = min(batch_size, n_files - done)
        imgs, labels, paths, shapes = source.get_next_batch(b)
        targets = []
        for k, lb in enumerate(labels):
            t = torch.from_numpy(np.asarray(lb, np.float32)).reshape(-1, 6).clone()
            t[:, 0] = k
            if single_cls:
                t[:, 1] = 0
            targets.append(t)
        done += b
        yield torch.stack(imgs), torch.cat(targets, 0), paths, shapes


class _Engines:
    """The detector of run_eval over YoloEngines of fixed batch sizes: each batch goes to the engine of its size."""

    def __init__(self, engines):
        self.engines = engines

    def __call__(self, x):
        return self.engines[int(x.shape[0])](x)

    def check_chains(self, sync=False):
        for e in self.engines.values():
            e.check_chains(sync=sync)


def main(argv=None):
    a = parse_args(argv)
    import torch

    from ..agent import Agent
    from ..config import cfg
    from ..data import ImageFolderSource
    from ..rawcal import calibration_from_options
    from ..yolo import DetectionModel, YoloEngine
    from ..yolo.checkpoint import load_detector_checkpoint, load_isp_checkpoint
    from . import writers
    from .harness import run_eval

    source, yaml_names, yaml_nc = resolve_data(a.data, a.task)
    if not torch.cuda.is_available():
        raise SystemExit("adaptiveisp_amd.val needs a HIP device (the ISP and detector kernels have no CPU path)")
    dev = torch.device("cuda:0")
    torch.manual_seed(a.seed)

    # ---- models
    if a.detector_ckpt:
        det = load_detector_checkpoint(a.detector_ckpt)
        names = det.names if isinstance(det.names, dict) else dict(enumerate(det.names))
        ckpt_nc = len(names)
    else:
        print(f"WARNING: no --detector-ckpt: a randomly initialised {a.detector_cfg} (the numbers mean nothing; smoke runs only)")
        det = DetectionModel(cfg=a.detector_cfg, nc=yaml_nc or 80)
        names, ckpt_nc = None, None
    if yaml_nc is not None and ckpt_nc is not None and yaml_nc != ckpt_nc and not a.single_cls:
        raise SystemExit(f"{a.detector_ckpt} ({ckpt_nc} classes) was trained on different data than --data {a.data} "
                         f"({yaml_nc} classes)")
    nc = 1 if a.single_cls else (yaml_nc or ckpt_nc or det.model[-1].nc)
    names = yaml_names or names or {i: str(i) for i in range(det.model[-1].nc)}
    det = det.to(dev).eval()
    agent = Agent(cfg, shape=(6 + len(cfg.filters), 64, 64), device=dev).to(dev)
    load_isp_checkpoint(a.isp_ckpt, agent, map_location=dev)
    agent.eval()

    # ---- data and detector engines (one per batch size that occurs)
    src = ImageFolderSource(source, a.img_size, dev, data_name=a.data_name, add_noise=a.add_noise,
                            brightness_range=a.bri_range, noise_level=a.noise_level, use_linear=a.use_linear,
                            seed=a.seed, workers=a.workers, resize=a.resize, sensor=a.sensor, cfa=a.cfa,
                            raw_bits=a.raw_bits, black_level=a.black_level, demosaic=a.demosaic,
                            raw_gains=tuple(a.raw_gains), raw_calibration=calibration_from_options(a.raw_cal, a.raw_dpc, a.cfa),
                            raw_meta=a.raw_meta)
    if src.raw_calibration is not None or src.raw_meta:
        print(f"data: {src.describe()}")
    n_files = len(src)
    engines = {}
    for b in {min(a.batch_size, n_files), n_files % a.batch_size or a.batch_size}:
        engines[b] = YoloEngine(det, b, a.img_size, a.img_size, device=dev)
        if a.tune_cache:
            engines[b].autotune(cache=a.tune_cache)
    detector = _Engines(engines)

    # ---- outputs
    save_dir = increment_path(os.path.join(a.project, a.name), a.exist_ok)
    os.makedirs(os.path.join(save_dir, "labels") if a.save_txt else save_dir, exist_ok=True)
    image_dir = os.path.join(save_dir, "img_results") if a.save_image else None
    if image_dir:
        for i in range(a.steps):
            os.makedirs(os.path.join(image_dir, f"step-{i}"), exist_ok=True)
    class_map = writers.coco80_to_coco91_class()
    jdict = []

    def on_image(path, predn, shape):
        if a.save_txt:
            stem = os.path.splitext(os.path.basename(path))[0]
            writers.save_one_txt(predn, a.save_conf, shape, os.path.join(save_dir, "labels", stem + ".txt"))
        if a.save_json:
            writers.save_one_json(predn, jdict, path, class_map)

    # ---- the loop
    writer = writers.ImageWriter() if image_dir else None
    np.random.seed(a.seed)                                  # the z noise of every step (util.get_noise)
    torch.cuda.synchronize(dev)
    t0 = time.perf_counter()
    finished = False
    try:
        res = run_eval(agent, detector, _batches(src, n_files, a.batch_size, a.single_cls), cfg, steps=a.steps,
                       conf_thres=a.conf_thres, iou_thres=a.iou_thres, max_det=a.max_det, single_cls=a.single_cls,
                       pipeline=a.pipeline, records_path=os.path.join(save_dir, "records.txt"), nc=nc,
                       param_dir=os.path.join(save_dir, "param_results") if a.save_param else None, graph=a.graph,
                       image_dir=image_dir, image_writer=writer,
                       on_image=on_image if (a.save_txt or a.save_json) else None, match=a.match, nms=a.nms,
                       confusion=True if a.confusion else None)
        torch.cuda.synchronize(dev)
        dt = time.perf_counter() - t0
        finished = True
    finally:
        # every pending image is written before the process exits; a failed write is raised only if the loop itself
        # succeeded, so it never hides the loop's own error
        if writer is not None:
            writer.close(raise_errors=finished)
        src.close()

    # ---- report
    nt, seen = res["nt"], res["seen"]
    print(HEADER)
    print(ROW % ("all", seen, nt.sum(), res["mp"], res["mr"], res["map50"], res["map75"], res["map"]))
    if nt.sum() == 0:
        print(f"WARNING: no labels found in the {a.task} set, can not compute metrics without labels")
    ap, rows = res["ap"], []
    for i, c in enumerate(res["ap_class"]):
        c = int(c)
        rows.append(dict(name=names.get(c, str(c)), images=seen, instances=int(nt[c]) if c < len(nt) else 0,
                         p=float(res["p"][i]), r=float(res["r"][i]), ap50=float(ap[i, 0]), ap75=float(ap[i, 5]),
                         ap=float(ap[i].mean())))
    if (a.verbose or nc < 50) and nc > 1:
        for row in rows:
            print(ROW % (row["name"], row["images"], row["instances"], row["p"], row["r"], row["ap50"], row["ap75"], row["ap"]))
    if a.confusion:
        cmat = res["confusion"]
        writers.save_confusion_csv(cmat, names, os.path.join(save_dir, "confusion_matrix.csv"))
        if a.verbose:
            print(("%22s" + "%11s" * 4) % ("Class", "Correct", "As other", "Backgr.", "Missed"))
            for c in range(nc):
                print(("%22s" + "%11i" * 4) % (names.get(c, str(c)), cmat[c, c], cmat[c, :nc].sum() - cmat[c, c], cmat[c, nc],
                                               cmat[nc, c]))
    ms = dt / max(seen, 1) * 1e3
    print(f"Speed: {ms:.1f} ms per image (ISP episode, detector, NMS, matching; data loading included) at shape "
          f"{(a.batch_size, 3, a.img_size, a.img_size)}")
    if a.save_json:
        stem = os.path.splitext(os.path.basename(a.detector_ckpt))[0] if a.detector_ckpt else ""
        with open(os.path.join(save_dir, f"{stem}_predictions.json"), "w") as f:
            json.dump(jdict, f)
    args = {k: v for k, v in vars(a).items()}
    with open(os.path.join(save_dir, "results.json"), "w") as f:
        json.dump(dict(mp=res["mp"], mr=res["mr"], map50=res["map50"], map75=res["map75"], map=res["map"], seen=seen,
                       instances=int(nt.sum()), classes=rows, ms_per_image=round(ms, 3), save_dir=save_dir, args=args),
                  f, indent=1)
    print(f"Results saved to {save_dir}")
    return res


if __name__ == "__main__":
    main()
