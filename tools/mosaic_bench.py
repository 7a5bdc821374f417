#!/usr/bin/env python3
"""adaisp_mosaic_u8 beside adaisp_augment_u8: 8 frames of 512 x 512, sources of 512 x 512 out of a pool of 32,
  mosaic_four      one layer of four tiles around a drawn centre, drawn maps (10 degrees, shear 5, scale 0.5, translate 0.1,
                   flips) and HSV tables: the mosaic = 1 training case
  mosaic_mixup     two such layers blended with a drawn ratio: the mixup case (twice the gathers)
  mosaic_one_tile  one layer of one tile filling the frame, the maps and tables of `augment`, launched with n_layers = 1: what
                   a single image costs when it rides in the mosaic launch
  augment          adaisp_augment_u8 on the same images, maps and tables (the two write the same bytes; checked once)
The arms alternate in one process, `--rounds` rounds of `--reps` launches each between a pair of device events, after a
discarded warm-up round; inputs rotate over `--bufs` staged pools. One JSON line: the median microseconds of each arm over
the rounds, their spread, the ratios to `augment`, the source bytes a batch of each kind stages, and the sha256 of the frames
each arm writes from the first pool (taken once, outside the timed loops: two builds of the kernel compare by it).
    python tools/mosaic_bench.py [--reps 200] [--rounds 7] [--bufs 2] [--out FILE]"""
import argparse
import hashlib
import json
import os
import random
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
B, S, POOL = 8, 512, 32


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=200)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--bufs", type=int, default=2)
    ap.add_argument("--out", default=None, help="also append the JSON line to this file")
    a = ap.parse_args()
    import torch
    sys.path.insert(0, ROOT)
    from adaptiveisp_amd import _lib
    from adaptiveisp_amd.augment import (Hyp, draw, draw_mosaic, fill_mosaic_layer, fill_single_layer, fixed_inverse, mix_q16,
                                         mosaic_tiles)
    if not torch.cuda.is_available():
        raise SystemExit("tools/mosaic_bench.py measures on the HIP device; there is none")
    rs, rng = np.random.RandomState(0), random.Random(0)
    hyp = Hyp(degrees=10, shear=5, scale=0.5, translate=0.1, flipud=0.5)
    draws = [draw(hyp, rng, rs, S) for _ in range(B)]
    luts = torch.from_numpy(np.stack([d.luts.reshape(-1) for d in draws])).cuda()
    image = S * S * 3

    def mosaic_records(layers):
        rec = np.zeros(B, _lib.MOSAIC_DESC)
        rec["n_layers"], rec["mix"] = layers, _lib.MOSAIC_MIX_ONE
        for b, d in enumerate(draws):
            rec[b]["lut"] = b
            if layers == 2:
                rec[b]["mix"] = mix_q16(rs.beta(32.0, 32.0))
            for l in range(layers):
                mz = draw_mosaic(hyp, rng, rs, S, POOL, (8 * l + b) % POOL)
                lay, sizes = rec[b]["layer"][l], [(S, S)] * 4
                fill_mosaic_layer(lay, fixed_inverse(mz.M, d.flipud, d.fliplr, S), sizes, mosaic_tiles(sizes, mz.centre, S))
                lay["tile"]["src_offset"] = np.array(mz.indices) * image
        return rec

    one = np.zeros(B, _lib.MOSAIC_DESC)
    aug = np.zeros(B, _lib.AUGMENT_DESC)
    one["n_layers"], one["mix"] = 1, _lib.MOSAIC_MIX_ONE
    for b, d in enumerate(draws):
        m = fixed_inverse(d.M, d.flipud, d.fliplr, S)
        aug[b]["src_offset"], aug[b]["h"], aug[b]["w"], aug[b]["m"], aug[b]["lut"] = b * image, S, S, m, b
        fill_single_layer(one[b]["layer"][0], m, S, S, 0, 0)
        one[b]["lut"], one[b]["layer"][0]["tile"][0]["src_offset"] = b, b * image
    host = {"mosaic_four": mosaic_records(1), "mosaic_mixup": mosaic_records(2), "mosaic_one_tile": one, "augment": aug}
    dev = {k: torch.from_numpy(v.view(np.uint8).copy()).cuda() for k, v in host.items()}
    srcs = [torch.from_numpy(rs.randint(0, 256, POOL * image).astype(np.uint8)).cuda() for _ in range(a.bufs)]
    frames = torch.empty(B * image, dtype=torch.uint8, device="cuda")
    for k in host:
        if k != "augment":
            _lib._check_mosaic_records(host[k], POOL * image, B)
    same = torch.equal(_lib.mosaic_u8(srcs[0], dev["mosaic_one_tile"], luts, S, n_layers=1).reshape(-1),
                       _lib.augment_u8(srcs[0], dev["augment"], luts, S, fill=0).reshape(-1))

    def run(key):
        if key == "augment":
            return lambda i: _lib.augment_u8(srcs[i % a.bufs], dev[key], luts, S, fill=0, out=frames)
        layers = 2 if key == "mosaic_mixup" else 1
        return lambda i: _lib.mosaic_u8(srcs[i % a.bufs], dev[key], luts, S, n_layers=layers, out=frames)

    def timed(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for i in range(a.reps):
            fn(i)
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) / a.reps * 1e3

    keys = list(host)
    sha = {}
    for k in keys:                                              # each arm's frames from the first pool, outside the timed loops
        run(k)(0)
        sha[k] = hashlib.sha256(frames.cpu().numpy().tobytes()).hexdigest()
    t = {k: [] for k in keys}
    for r in range(a.rounds + 1):                               # round 0 is the warm-up
        for k in keys[r % len(keys):] + keys[:r % len(keys)]:   # the order rotates from round to round
            us = timed(run(k))
            if r:
                t[k].append(us)
    med = {k: float(np.median(v)) for k, v in t.items()}
    line = dict(B=B, S=S, reps=a.reps, rounds=a.rounds, timing="device events, launches included", device=torch.cuda.get_device_name(0),
                one_tile_equals_augment=bool(same))
    for k in keys:
        line[k + "_us"] = round(med[k], 2)
        line[k + "_min_max_us"] = [round(min(t[k]), 2), round(max(t[k]), 2)]
        line[k + "_over_augment"] = round(med[k] / med["augment"], 3)
        line[k + "_sha256"] = sha[k]
    line["record_bytes"] = dict(mosaic=_lib.MOSAIC_DESC.itemsize, augment=_lib.AUGMENT_DESC.itemsize)
    line["staged_source_MB_per_batch"] = dict(augment=round(B * image / 1e6, 1), mosaic_four=round(4 * B * image / 1e6, 1),
                                              mosaic_mixup=round(8 * B * image / 1e6, 1))
    text = json.dumps(line)
    print(text, flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "a") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
