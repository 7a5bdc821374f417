#!/usr/bin/env python3
"""Interleaved A/B of the RL trainer's input: synthetic images vs an image dataset as `lod` and as `coco --add-noise`
(adaptiveisp_amd/data.py). Writes a seeded toy dataset (JPEG and PNG at mixed sizes, YOLO labels, some images without)
into a temporary directory, then runs `python -m adaptiveisp_amd.train` for the three arms in interleaved fresh child
processes, each under its own time limit, and prints ms_per_iter per run and the median per arm (one JSON line each).
    python tools/train_data_ab.py [--rounds 3] [--iters 200] [--batch 8] [--size 512] [--images 64] [--workers 4]
                                  [--photo-sizes] [--resize host|device|both]
By default the images are S on the longer side, so the decode is PIL alone; --photo-sizes makes load_image's area
resampler run on every image (the numpy restatement of cv2's INTER_AREA, val/loader.py: ~1 s per 640 x 480 image on one
core), which the trainer then waits for with `--resize host`. `--resize device` runs the dataset arms with the resample on
the device (adaisp_resize_u8: the worker threads only decode); `both` runs the host and the device arms. The tool also
prints the host decode rate with `workers` threads: the full host path (decode + resample + letterbox) and, for the
device arms, the decode alone."""
import argparse
import json
import os
import statistics
import subprocess
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


PHOTO_SIZES = [(480, 640), (640, 480), (375, 500), (427, 640), (512, 512), (720, 1280), (333, 500), (640, 427)]


def write_dataset(root, n, S, photo=False, seed=0):
    """n images: at S on the longer side (no resampling in load_image) or, with `photo`, at camera / COCO-like sizes."""
    from PIL import Image
    rs = np.random.RandomState(seed)
    os.makedirs(os.path.join(root, "images"))
    os.makedirs(os.path.join(root, "labels"))
    sizes = PHOTO_SIZES if photo else [(S * 3 // 4, S), (S, S * 3 // 4), (S, S), (S * 2 // 3, S)]
    for i in range(n):
        h, w = sizes[i % len(sizes)]
        # smooth content (a JPEG of white noise decodes at an unrepresentative speed)
        yy, xx = np.mgrid[0:h, 0:w].astype(np.float32)
        f = rs.uniform(0.005, 0.05, 3)
        im = np.stack([127 + 120 * np.sin(f[c] * xx + f[(c + 1) % 3] * yy + c) for c in range(3)], -1)
        im = np.clip(im + rs.normal(0, 8, im.shape), 0, 255).astype(np.uint8)
        ext = "jpg" if i % 3 else "png"
        Image.fromarray(im).save(os.path.join(root, "images", f"{i:05d}.{ext}"), **({"quality": 90} if ext == "jpg" else {}))
        if i % 7:
            with open(os.path.join(root, "labels", f"{i:05d}.txt"), "w") as fh:
                for _ in range(1 + i % 4):
                    fh.write(f"{rs.randint(80)} {rs.uniform(0.2, 0.8):.5f} {rs.uniform(0.2, 0.8):.5f} "
                             f"{rs.uniform(0.05, 0.3):.5f} {rs.uniform(0.05, 0.3):.5f}\n")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--size", type=int, default=512)
    ap.add_argument("--images", type=int, default=64)
    ap.add_argument("--workers", type=int, default=4)
    ap.add_argument("--photo-sizes", action="store_true", help="camera-sized images (load_image resamples every one)")
    ap.add_argument("--resize", default="host", choices=("host", "device", "both"),
                    help="where the dataset arms resample (both: one arm of each per dataset kind)")
    ap.add_argument("--timeout", type=int, default=600, help="seconds per child")
    a = ap.parse_args()
    with tempfile.TemporaryDirectory() as tmp:
        write_dataset(tmp, a.images, a.size, a.photo_sizes)
        # host decode rate (what the source's worker threads can deliver), before any child starts
        sys.path.insert(0, ROOT)
        import time
        from concurrent.futures import ThreadPoolExecutor
        from adaptiveisp_amd.val.loader import imread_bgr, list_images, load_letterboxed
        files = list_images(tmp)[:16]
        rates = {}
        for kind, fn in (("host_resize", lambda f: load_letterboxed(f, a.size)), ("decode_only", imread_bgr)):
            if kind == "host_resize" and a.resize == "device":
                continue
            with ThreadPoolExecutor(max(a.workers, 1)) as ex:
                t0 = time.perf_counter()
                list(ex.map(fn, files))
                rates[kind] = round(len(files) / (time.perf_counter() - t0), 1)
        print(json.dumps({"decode_images_per_s": rates, "workers": a.workers, "photo_sizes": a.photo_sizes}), flush=True)
        common = ["--batch", str(a.batch), "--size", str(a.size), "--iters", str(a.iters + a.warmup), "--warmup", str(a.warmup)]
        arms = {"synthetic": []}
        for resize in (("host", "device") if a.resize == "both" else (a.resize,)):
            tag = "" if resize == "host" else "_device"
            arms["lod" + tag] = ["--data", tmp, "--data-name", "lod", "--data-workers", str(a.workers), "--resize", resize]
            arms["coco_noise" + tag] = ["--data", tmp, "--data-name", "coco", "--add-noise", "--data-workers",
                                        str(a.workers), "--resize", resize]
        res = {k: [] for k in arms}
        for r in range(a.rounds):
            for name, extra in arms.items():
                cmd = ["timeout", "-k", "10", str(a.timeout), sys.executable, "-m", "adaptiveisp_amd.train"] + common + extra
                p = subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True)
                if p.returncode != 0:
                    print(json.dumps({"arm": name, "round": r, "returncode": p.returncode, "stderr": p.stderr[-2000:]}), flush=True)
                    raise SystemExit(p.returncode)
                line = json.loads([ln for ln in p.stdout.splitlines() if ln.startswith("{")][-1])
                res[name].append(line["ms_per_iter"])
                print(json.dumps({"arm": name, "round": r, "ms_per_iter": line["ms_per_iter"], "data": line["data"]}), flush=True)
        base = statistics.median(res["synthetic"])
        print(json.dumps({"median_ms_per_iter": {k: statistics.median(v) for k, v in res.items()},
                          "vs_synthetic": {k: round(statistics.median(v) / base - 1, 4) for k, v in res.items()},
                          "runs": res, "batch": a.batch, "size": a.size, "iters": a.iters, "workers": a.workers,
                          "photo_sizes": a.photo_sizes, "resize": a.resize}), flush=True)


if __name__ == "__main__":
    main()
