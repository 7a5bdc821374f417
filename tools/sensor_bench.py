#!/usr/bin/env python3
"""The simulated Bayer sensor against the conversion it extends: adaisp_unprocess alone (3 B/px in, 12 out = 15 B/px of
the S x S frame) and adaisp_unprocess_bayer + adaisp_demosaic_rects (3 + 2, then 2 + 12 = 19 B/px), both with noise, at
  frame   8 images of 512 x 512 filling their 512 x 512 frames
  photo   one batch of 4 photo-sized images (3000 x 4000 decoded) as they reach the kernels: 384 x 512 in a 512 frame
The two forms alternate in one process, `--rounds` rounds of `--reps` launches each between a pair of device events, after
a discarded warm-up round; inputs rotate over `--bufs` staged batches. Per case one JSON line: the median microseconds of
each form over the rounds, their spread, the achieved GB/s against the algorithmic bytes above (frame bytes: the pad is
written too), and pair / unprocess against the 19 / 15 the byte counts predict.
    python tools/sensor_bench.py [--reps 200] [--rounds 7] [--bufs 4] [--out FILE]"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = {"frame": dict(B=8, S=512, h=512, w=512), "photo": dict(B=4, S=512, h=384, w=512)}
RGB_BYTES, PAIR_BYTES = 15, 19                                  # per pixel of the frame


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=200)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--bufs", type=int, default=4)
    ap.add_argument("--out", default=None, help="also append the JSON lines to this file")
    a = ap.parse_args()
    import torch
    sys.path.insert(0, ROOT)
    from adaptiveisp_amd import _lib
    from adaptiveisp_amd.data import kernel_params, sample_unprocess_params
    if not torch.cuda.is_available():
        raise SystemExit("tools/sensor_bench.py measures on the HIP device; there is none")
    NF = _lib.UNP_UNPROCESS | _lib.UNP_NOISE
    for name, c in CASES.items():
        B, S, h, w = c["B"], c["S"], c["h"], c["w"]
        rs = np.random.RandomState(0)
        desc = np.zeros(B, _lib.UNPROCESS_DESC)
        for b in range(B):
            desc[b]["src_offset"], desc[b]["h"], desc[b]["w"] = b * h * w * 3, h, w
            desc[b]["top"], desc[b]["left"], desc[b]["serial"] = (S - h) // 2, (S - w) // 2, b
            desc[b]["p"] = kernel_params(sample_unprocess_params(rs, True, (0.1, 0.3)))
        d = torch.from_numpy(desc.view(np.uint8).copy()).cuda()
        srcs = [torch.from_numpy(rs.randint(0, 256, B * h * w * 3).astype(np.uint8)).cuda() for _ in range(a.bufs)]
        rgb = torch.empty((B, 3, S, S), device="cuda")
        plane = torch.empty((B, S, S), dtype=torch.int16, device="cuda")
        out = torch.empty((B, 3, S, S), device="cuda")
        lv = dict(pattern="RGGB", black_level=64, white_level=4095)

        def one(i):
            _lib.unprocess(srcs[i % a.bufs], d, S, seed=1, flags=NF, out=rgb)

        def pair(i):
            _lib.unprocess_bayer(srcs[i % a.bufs], d, S, seed=1, flags=NF, out=plane, **lv)
            _lib.demosaic_rects(plane, d, out=out, **lv)

        def sensor(i):
            _lib.unprocess_bayer(srcs[i % a.bufs], d, S, seed=1, flags=NF, out=plane, **lv)

        def timed(fn):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for i in range(a.reps):
                fn(i)
            e1.record()
            torch.cuda.synchronize()
            return e0.elapsed_time(e1) / a.reps * 1e3

        t = {"unprocess": [], "pair": [], "sensor": []}
        for r in range(a.rounds + 1):                           # round 0 is the warm-up
            for key, fn in (("unprocess", one), ("pair", pair), ("sensor", sensor)):
                us = timed(fn)
                if r:
                    t[key].append(us)
        med = {k: float(np.median(v)) for k, v in t.items()}
        px = B * S * S
        line = dict(case=name, B=B, S=S, image_hw=[h, w], reps=a.reps, rounds=a.rounds, timing="device events, launches included",
                    unprocess_us=round(med["unprocess"], 2), pair_us=round(med["pair"], 2), sensor_us=round(med["sensor"], 2),
                    demosaic_us_by_difference=round(med["pair"] - med["sensor"], 2),
                    unprocess_min_max_us=[round(min(t["unprocess"]), 2), round(max(t["unprocess"]), 2)],
                    pair_min_max_us=[round(min(t["pair"]), 2), round(max(t["pair"]), 2)],
                    unprocess_bytes=RGB_BYTES * px, pair_bytes=PAIR_BYTES * px,
                    unprocess_GBps=round(RGB_BYTES * px / med["unprocess"] / 1e3, 1),
                    pair_GBps=round(PAIR_BYTES * px / med["pair"] / 1e3, 1),
                    pair_over_unprocess=round(med["pair"] / med["unprocess"], 3), expected_from_bytes=round(PAIR_BYTES / RGB_BYTES, 3))
        text = json.dumps(line)
        print(text, flush=True)
        if a.out:
            os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
            with open(a.out, "a") as f:
                f.write(text + "\n")


if __name__ == "__main__":
    main()
