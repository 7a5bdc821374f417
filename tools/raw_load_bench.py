#!/usr/bin/env python3
"""The raw-capture loader against the whole-frame demosaic of the same planes: adaisp_raw_load (native uint16 planes ->
the letterboxed [8,3,512,512] batch in one launch: demosaic, gains, area resample, placement) and adaisp_demosaic_ex (the
same planes -> [8,3,H,W] fp32, what a loader without the fused kernel would have to run first), at
  12mp    8 planes of 3000 x 4000  -> 384 x 512 in a 512 frame
  1080p   8 planes of 1080 x 1920  -> 288 x 512 in a 512 frame
with both demosaics. Both read 2 B per native pixel; the loader writes 12 B per pixel of the batch, the whole-frame
demosaic 12 B per native pixel. The four (entry, method) pairs alternate in one process, `--rounds` rounds of `--reps`
launches each between a pair of device events, after a discarded warm-up round; the C entries are called directly and
inputs and outputs rotate over `--bufs` buffers. Per case and method one JSON line: the median microseconds of each entry
over the rounds, their spread, the achieved GB/s over each entry's algorithmic bytes (plane bytes read + bytes written),
and raw_load / demosaic. These are event times over back-to-back launches, not kernel times.
    python tools/raw_load_bench.py [--reps 20] [--rounds 7] [--bufs 3] [--out FILE]"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
S, B = 512, 8
CASES = (("12mp", 3000, 4000), ("1080p", 1080, 1920))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--bufs", type=int, default=3)
    ap.add_argument("--out", default=None, help="also append the JSON lines to this file")
    a = ap.parse_args()
    import torch
    sys.path.insert(0, ROOT)
    from adaptiveisp_amd import _lib
    from adaptiveisp_amd.resize import RawTapPlan
    from adaptiveisp_amd.val.loader import letterboxed_geometry
    if not torch.cuda.is_available():
        raise SystemExit("tools/raw_load_bench.py measures on the HIP device; there is none")
    L = _lib.load()
    rs = np.random.RandomState(0)
    black, white, pat = 64.0, 4095.0, 0

    for name, H, W in CASES:
        _, unpad, place, _frame, *_rest = letterboxed_geometry(H, W, S)
        plan = RawTapPlan()
        for b in range(B):
            plan.add((H, W), unpad, place, b * H * W * 2, (1.9, 1.0, 1.6))
        desc = torch.from_numpy(plan.descriptors().view(np.uint8).copy()).cuda()
        tabs = torch.from_numpy(plan.table().copy()).cuda()
        raws = [torch.from_numpy(rs.randint(0, 4096, (B, H, W)).astype(np.uint16).view(np.int16)).cuda() for _ in range(a.bufs)]
        small = [torch.empty((B, 3, S, S), device="cuda") for _ in range(a.bufs)]
        full = [torch.empty((B, 3, H, W), device="cuda") for _ in range(a.bufs)]
        plane_bytes, words = B * H * W * 2, tabs.numel()

        def call(entry, method, i):
            r = raws[i % a.bufs].data_ptr()
            if entry == "raw_load":
                return L.adaisp_raw_load(r, plane_bytes, desc.data_ptr(), tabs.data_ptr(), words, small[i % a.bufs].data_ptr(),
                                         B, S, pat, method, black, white, None)
            return L.adaisp_demosaic_ex(r, full[i % a.bufs].data_ptr(), B, H, W, pat, method, black, white, None)

        def timed(entry, method):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for i in range(a.reps):
                if call(entry, method, i) != 0:
                    raise SystemExit(f"{name}: {entry} method {method} was refused")
            e1.record()
            torch.cuda.synchronize()
            return e0.elapsed_time(e1) / a.reps * 1e3

        keys = [(e, m) for m in ("bilinear", "mhc") for e in ("raw_load", "demosaic")]
        t = {k: [] for k in keys}
        for r in range(a.rounds + 1):                           # round 0 is the warm-up
            for k in keys:
                us = timed(k[0], _lib.DEMOSAIC[k[1]])
                if r:
                    t[k].append(us)
        nbytes = {"raw_load": plane_bytes + B * 3 * S * S * 4, "demosaic": plane_bytes + B * 3 * H * W * 4}
        for m in ("bilinear", "mhc"):
            med = {e: float(np.median(t[(e, m)])) for e in ("raw_load", "demosaic")}
            line = dict(case=name, B=B, plane_hw=[H, W], S=S, image_hw=list(unpad), method=m, reps=a.reps, rounds=a.rounds,
                        bufs=a.bufs, timing="device events, launches included",
                        raw_load_us=round(med["raw_load"], 1), demosaic_us=round(med["demosaic"], 1),
                        raw_load_min_max_us=[round(min(t[("raw_load", m)]), 1), round(max(t[("raw_load", m)]), 1)],
                        demosaic_min_max_us=[round(min(t[("demosaic", m)]), 1), round(max(t[("demosaic", m)]), 1)],
                        raw_load_bytes=nbytes["raw_load"], demosaic_bytes=nbytes["demosaic"],
                        raw_load_GBps=round(nbytes["raw_load"] / med["raw_load"] / 1e3, 1),
                        demosaic_GBps=round(nbytes["demosaic"] / med["demosaic"] / 1e3, 1),
                        raw_load_over_demosaic=round(med["raw_load"] / med["demosaic"], 3))
            text = json.dumps(line)
            print(text, flush=True)
            if a.out:
                os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
                with open(a.out, "a") as f:
                    f.write(text + "\n")
        del raws, small, full


if __name__ == "__main__":
    main()
