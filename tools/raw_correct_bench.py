#!/usr/bin/env python3
"""adaisp_raw_correct (the calibration pass in front of adaisp_raw_load) on batches of 8 planes at a photo size against
the copy ceiling: the event-timed mean per launch with and without defect correction and lens shading, and a
device-to-device copy of the same plane bytes timed the same way (the kernel reads and writes 2 B per sample, as the copy
does). Batches rotate over `--bufs` buffers so that the working set exceeds the 256 MB last-level cache. One JSON line.
    python tools/raw_correct_bench.py [--reps 100] [--B 8] [--H 3000] [--W 4000] [--bufs 4] [--grid 13 17] [--dpc 40]"""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from adaptiveisp_amd import _lib  # noqa: E402
from adaptiveisp_amd.rawcal import fill_rawfix, level_scale  # noqa: E402


def _time(fn, reps):
    for i in range(10):
        fn(i)
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for i in range(reps):
        fn(i)
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps * 1e3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=100)
    ap.add_argument("--B", type=int, default=8)
    ap.add_argument("--H", type=int, default=3000)
    ap.add_argument("--W", type=int, default=4000)
    ap.add_argument("--bufs", type=int, default=4)
    ap.add_argument("--grid", type=int, nargs=2, default=(13, 17))
    ap.add_argument("--dpc", type=int, default=40)
    a = ap.parse_args()
    plane = a.H * a.W * 2
    stride = (plane + 15) // 16 * 16
    nbytes = a.B * stride
    g = torch.Generator(device="cuda").manual_seed(0)
    ins = [torch.randint(64, 4096, (nbytes // 2,), device="cuda", generator=g, dtype=torch.int32).to(torch.int16)
           .view(torch.uint8) for _ in range(a.bufs)]
    outs = [torch.empty(nbytes, dtype=torch.uint8, device="cuda") for _ in range(a.bufs)]
    gh, gw = a.grid
    yy, xx = np.mgrid[0:gh, 0:gw]
    table = np.broadcast_to(1.0 + ((yy / (gh - 1) - 0.5) ** 2 + (xx / (gw - 1) - 0.5) ** 2), (4, gh, gw)).astype(np.float32)
    gains = torch.from_numpy(np.ascontiguousarray(table).reshape(-1)).cuda()
    black = (60.0, 64.0, 66.0, 71.0)

    def records(dpc, shade):
        rec = np.zeros(a.B, _lib.RAWFIX_DESC)
        for b in range(a.B):
            fill_rawfix(rec[b], (a.H, a.W), b * stride, b * stride, black, level_scale(black, 4000, 64, 4095), 64, dpc,
                        (0, gh, gw) if shade else None)
        return torch.from_numpy(rec.view(np.uint8)).cuda()

    res = {"B": a.B, "H": a.H, "W": a.W, "grid": [gh, gw], "dpc": a.dpc, "bytes": 2 * a.B * plane}
    copy_us = _time(lambda i: outs[i % a.bufs].copy_(ins[(i + 1) % a.bufs]), a.reps)
    res["copy_us"] = round(copy_us, 2)
    res["copy_TBps"] = round(2 * nbytes / (copy_us * 1e-6) / 1e12, 2)
    for name, dpc, shade in (("levels", -1, False), ("dpc", a.dpc, False), ("shading", -1, True), ("dpc_shading", a.dpc, True)):
        desc = records(dpc, shade)
        us = _time(lambda i: _lib.raw_correct(ins[(i + 1) % a.bufs], desc, gains if shade else None, out=outs[i % a.bufs]),
                   a.reps)
        res[name + "_us"] = round(us, 2)
        res[name + "_over_copy"] = round(us / copy_us, 3)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
