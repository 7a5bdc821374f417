#!/usr/bin/env python3
"""adaisp_augment_u8 beside the launch it feeds: 8 images of 512 x 512 filling their 512 x 512 frames,
  augment            drawn maps (10 degrees, shear 5, scale 0.5, translate 0.1, flips) and HSV tables: the training case
  augment_no_tables  the same maps, lut = -1: the gathers and stores alone (the tables' cost is the difference)
  augment_identity   identity maps, lut = -1: the same stores with coalesced reads (the gathers' cost is the difference)
  unprocess          adaisp_unprocess with noise on the 8 frames the first arm wrote, for scale
The arms alternate in one process, `--rounds` rounds of `--reps` launches each between a pair of device events, after a
discarded warm-up round; inputs rotate over `--bufs` staged batches. One JSON line: the median microseconds of each arm over
the rounds, their spread, the GB/s against the algorithmic bytes (augment: 3 B/px read + 3 written; unprocess: 3 + 12), and the
sha256 of the frames each augment arm writes from the first batch (taken once, outside the timed loops).
    python tools/augment_bench.py [--reps 200] [--rounds 7] [--bufs 4] [--out FILE]"""
import argparse
import hashlib
import json
import os
import random
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
B, S = 8, 512
AUG_BYTES, UNP_BYTES = 6, 15                                    # per pixel of the frame


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=200)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--bufs", type=int, default=4)
    ap.add_argument("--out", default=None, help="also append the JSON line to this file")
    a = ap.parse_args()
    import torch
    sys.path.insert(0, ROOT)
    from adaptiveisp_amd import _lib
    from adaptiveisp_amd.augment import Hyp, draw, fixed_inverse
    from adaptiveisp_amd.data import kernel_params, sample_unprocess_params
    if not torch.cuda.is_available():
        raise SystemExit("tools/augment_bench.py measures on the HIP device; there is none")
    rs, rng = np.random.RandomState(0), random.Random(0)
    hyp = Hyp(degrees=10, shear=5, scale=0.5, translate=0.1, flipud=0.5)
    draws = [draw(hyp, rng, rs, S) for _ in range(B)]
    luts = torch.from_numpy(np.stack([d.luts.reshape(-1) for d in draws])).cuda()

    def records(identity, tables):
        rec = np.zeros(B, _lib.AUGMENT_DESC)
        for b, d in enumerate(draws):
            rec[b]["src_offset"], rec[b]["h"], rec[b]["w"] = b * S * S * 3, S, S
            rec[b]["m"] = (65536, 0, 0, 0, 65536, 0) if identity else fixed_inverse(d.M, d.flipud, d.fliplr, S)
            rec[b]["lut"] = b if tables else -1
        return torch.from_numpy(rec.view(np.uint8).copy()).cuda()

    arms = {"augment": records(False, True), "augment_no_tables": records(False, False), "augment_identity": records(True, False)}
    srcs = [torch.from_numpy(rs.randint(0, 256, B * S * S * 3).astype(np.uint8)).cuda() for _ in range(a.bufs)]
    frames = torch.empty(B * S * S * 3, dtype=torch.uint8, device="cuda")
    udesc = np.zeros(B, _lib.UNPROCESS_DESC)
    for b in range(B):
        udesc[b]["src_offset"], udesc[b]["h"], udesc[b]["w"], udesc[b]["serial"] = b * S * S * 3, S, S, b
        udesc[b]["p"] = kernel_params(sample_unprocess_params(rs, True, (0.1, 0.3)))
    ud = torch.from_numpy(udesc.view(np.uint8).copy()).cuda()
    rgb = torch.empty((B, 3, S, S), device="cuda")
    NF = _lib.UNP_UNPROCESS | _lib.UNP_NOISE

    def run(key):
        if key == "unprocess":
            return lambda i: _lib.unprocess(frames, ud, S, seed=1, flags=NF, out=rgb)
        return lambda i: _lib.augment_u8(srcs[i % a.bufs], arms[key], luts, S, fill=0, out=frames)

    def timed(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for i in range(a.reps):
            fn(i)
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) / a.reps * 1e3

    keys = ["augment", "augment_no_tables", "augment_identity", "unprocess"]      # unprocess last: it reads the first arm's frames
    sha = {}
    for k in keys[:3]:                                          # each arm's frames from the first batch, outside the timed loops
        run(k)(0)
        sha[k] = hashlib.sha256(frames.cpu().numpy().tobytes()).hexdigest()
    t = {k: [] for k in keys}
    for r in range(a.rounds + 1):                               # round 0 is the warm-up
        for k in keys[:1] + keys[3:] + keys[1:3]:
            us = timed(run(k))
            if r:
                t[k].append(us)
    med = {k: float(np.median(v)) for k, v in t.items()}
    px = B * S * S
    line = dict(B=B, S=S, reps=a.reps, rounds=a.rounds, timing="device events, launches included", device=torch.cuda.get_device_name(0))
    for k in keys:
        line[k + "_us"] = round(med[k], 2)
        line[k + "_min_max_us"] = [round(min(t[k]), 2), round(max(t[k]), 2)]
        line[k + "_GBps"] = round((UNP_BYTES if k == "unprocess" else AUG_BYTES) * px / med[k] / 1e3, 1)
        if k in sha:
            line[k + "_sha256"] = sha[k]
    line["tables_us_by_difference"] = round(med["augment"] - med["augment_no_tables"], 2)
    line["gathers_us_by_difference"] = round(med["augment_no_tables"] - med["augment_identity"], 2)
    line["augment_over_unprocess"] = round(med["augment"] / med["unprocess"], 3)
    text = json.dumps(line)
    print(text, flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "a") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
