#!/usr/bin/env python3
"""adayolo_spp_fwd / adayolo_spp_bwd and what SPP costs the detector's forward:
  spp_fwd, spp_bwd      the two launches in the engine's layout (x / grad_x = channel slice 0, the pools / their gradients slices
                        1..3 of one [B,H,W,4C] bf16 tensor; the backward accumulates) at 8 x 23 x 40 x 512 (P5 of 8 x 720 x 1280,
                        the benchmark's shape) and at 4 x 68 x 120 x 512 (P5 of 4 x 2160 x 3840)
  engine_plain, engine_spp
                        YoloEngine forwards of yolov3 and yolov3-spp at 8 x 720 x 1280 with the tuning table (shapes it lacks
                        are measured, nothing is written back)
The arms alternate in one process, `--rounds` rounds of `--reps` runs each between a pair of device events, after a discarded
warm-up round. One JSON line: the median microseconds of each arm over the rounds, their spread, and engine_spp - engine_plain.
    python tools/spp_bench.py [--reps 100] [--rounds 7] [--out FILE]"""
import argparse
import ctypes
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHAPES = {"8x23x40x512": (8, 23, 40, 512), "4x68x120x512": (4, 68, 120, 512)}
ENGINE = (8, 720, 1280)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=100)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--out", default=None, help="also append the JSON line to this file")
    a = ap.parse_args()
    import torch
    sys.path.insert(0, ROOT)
    from adaptiveisp_amd.yolo import YoloEngine, _lib, yolov3, yolov3_spp
    if not torch.cuda.is_available():
        raise SystemExit("tools/spp_bench.py measures on the HIP device; there is none")
    L = _lib.load()
    g = torch.Generator().manual_seed(0)
    arms = {}
    for name, (B, H, W, C) in SHAPES.items():
        act = torch.randn(B, H, W, 4 * C, generator=g).to(torch.bfloat16).cuda()
        grad = torch.randn(B, H, W, 4 * C, generator=g).to(torch.bfloat16).cuda()
        p = lambda t, off=0: ctypes.c_void_p(t.data_ptr() + 2 * off)                                # noqa: E731
        arms[f"spp_fwd_{name}"] = lambda act=act, s=(B, H, W, C): _lib.check(
            L.adayolo_spp_fwd(p(act), 4 * s[3], p(act, s[3]), 4 * s[3], *s, _lib.stream_ptr()), "adayolo_spp_fwd")
        arms[f"spp_bwd_{name}"] = lambda act=act, grad=grad, s=(B, H, W, C): _lib.check(
            L.adayolo_spp_bwd(p(act), 4 * s[3], p(grad, s[3]), 4 * s[3], p(grad), 4 * s[3], 1, *s, _lib.stream_ptr()), "adayolo_spp_bwd")
    cache = os.path.join(ROOT, "adaptiveisp_amd", "yolo", "tuning", "mi355x.json")
    img = torch.rand((ENGINE[0], 3, ENGINE[1], ENGINE[2]), generator=g).cuda()
    launches = {}
    for name, make in (("engine_plain", yolov3), ("engine_spp", yolov3_spp)):
        eng = YoloEngine(make().eval(), *ENGINE, device="cuda:0")
        eng.autotune(cache=cache, write=False)
        launches[name] = eng.num_launches()
        arms[name] = lambda eng=eng: eng(img)

    def timed(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(a.reps):
            fn()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) / a.reps * 1e3

    keys = list(arms)
    t = {k: [] for k in keys}
    for r in range(a.rounds + 1):                               # round 0 is the warm-up
        for k in keys[r % len(keys):] + keys[:r % len(keys)]:   # the order rotates from round to round
            us = timed(arms[k])
            if r:
                t[k].append(us)
    med = {k: float(np.median(v)) for k, v in t.items()}
    line = dict(reps=a.reps, rounds=a.rounds, timing="device events, launches included", device=torch.cuda.get_device_name(0),
                engine_shape=list(ENGINE), launches=launches)
    for k in keys:
        line[k + "_us"] = round(med[k], 2)
        line[k + "_min_max_us"] = [round(min(t[k]), 2), round(max(t[k]), 2)]
    line["engine_spp_minus_plain_us"] = round(med["engine_spp"] - med["engine_plain"], 2)
    text = json.dumps(line)
    print(text, flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "a") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
