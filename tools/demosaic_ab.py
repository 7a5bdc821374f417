#!/usr/bin/env python3
"""The two demosaics side by side: bilinear (ADAISP_DEMOSAIC_BILINEAR, the kernels of adaisp_demosaic /
adaisp_demosaic_rects) against the gradient-corrected one (ADAISP_DEMOSAIC_MHC), through adaisp_demosaic_ex /
adaisp_demosaic_rects_ex, at
  frame   8 x 720 x 1280, whole frame
  rects   8 x 512 x 512, every image filling its frame (the shape tools/sensor_bench.py times)
Both move 2 B/px in and 12 B/px out. The two methods alternate in one process, `--rounds` rounds of `--reps` launches each
between a pair of device events, after a discarded warm-up round; the C entries are called directly (no wrapper between
the launches) and inputs and outputs rotate over `--bufs` buffers. Per case one JSON line: the median microseconds of each
method over the rounds, their spread, the achieved GB/s over the algorithmic 14 B/px, that rate's share of the 8.0 TB/s
HBM peak, and mhc / bilinear. These are event times over back-to-back launches, not kernel times.
    python tools/demosaic_ab.py [--reps 200] [--rounds 7] [--bufs 4] [--out FILE]"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BYTES_PER_PX = 14
HBM_PEAK_GBPS = 8000.0


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
    if not torch.cuda.is_available():
        raise SystemExit("tools/demosaic_ab.py measures on the HIP device; there is none")
    L = _lib.load()
    rs = np.random.RandomState(0)
    black, white, pat = 64.0, 4095.0, 0

    def planes(B, H, W):
        return [torch.from_numpy(rs.randint(0, 4096, (B, H, W)).astype(np.uint16).view(np.int16)).cuda() for _ in range(a.bufs)]

    def case_frame():
        B, H, W = 8, 720, 1280
        raws = planes(B, H, W)
        outs = [torch.empty((B, 3, H, W), device="cuda") for _ in range(a.bufs)]
        ptrs = [(r.data_ptr(), o.data_ptr()) for r, o in zip(raws, outs)]

        def call(method, i):
            r, o = ptrs[i % a.bufs]
            return L.adaisp_demosaic_ex(r, o, B, H, W, pat, method, black, white, None)
        return dict(case="frame", B=B, H=H, W=W), B * H * W, call, (raws, outs)

    def case_rects():
        B, S = 8, 512
        desc = np.zeros(B, _lib.UNPROCESS_DESC)
        desc["h"], desc["w"] = S, S
        d = torch.from_numpy(desc.view(np.uint8).copy()).cuda()
        raws = planes(B, S, S)
        outs = [torch.empty((B, 3, S, S), device="cuda") for _ in range(a.bufs)]
        ptrs = [(r.data_ptr(), o.data_ptr()) for r, o in zip(raws, outs)]

        def call(method, i):
            r, o = ptrs[i % a.bufs]
            return L.adaisp_demosaic_rects_ex(r, d.data_ptr(), o, B, S, pat, method, black, white, None)
        return dict(case="rects", B=B, S=S, image_hw=[S, S]), B * S * S, call, (raws, outs, d)

    for make in (case_frame, case_rects):
        head, px, call, keep = make()

        def timed(method):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for i in range(a.reps):
                if call(method, i) != 0:
                    raise SystemExit(f"{head['case']}: method {method} was refused")
            e1.record()
            torch.cuda.synchronize()
            return e0.elapsed_time(e1) / a.reps * 1e3

        t = {"bilinear": [], "mhc": []}
        for r in range(a.rounds + 1):                           # round 0 is the warm-up
            for key in ("bilinear", "mhc"):
                us = timed(_lib.DEMOSAIC[key])
                if r:
                    t[key].append(us)
        med = {k: float(np.median(v)) for k, v in t.items()}
        gbps = {k: BYTES_PER_PX * px / med[k] / 1e3 for k in med}
        line = dict(**head, reps=a.reps, rounds=a.rounds, bufs=a.bufs, timing="device events, launches included",
                    bytes=BYTES_PER_PX * px,
                    bilinear_us=round(med["bilinear"], 2), mhc_us=round(med["mhc"], 2),
                    bilinear_min_max_us=[round(min(t["bilinear"]), 2), round(max(t["bilinear"]), 2)],
                    mhc_min_max_us=[round(min(t["mhc"]), 2), round(max(t["mhc"]), 2)],
                    bilinear_GBps=round(gbps["bilinear"], 1), mhc_GBps=round(gbps["mhc"], 1),
                    bilinear_share_of_hbm_peak=round(gbps["bilinear"] / HBM_PEAK_GBPS, 3),
                    mhc_share_of_hbm_peak=round(gbps["mhc"] / HBM_PEAK_GBPS, 3),
                    mhc_over_bilinear=round(med["mhc"] / med["bilinear"], 3))
        text = json.dumps(line)
        print(text, flush=True)
        if a.out:
            os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
            with open(a.out, "a") as f:
                f.write(text + "\n")
        del keep


if __name__ == "__main__":
    main()
