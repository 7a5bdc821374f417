#!/usr/bin/env python3
"""adaisp_export_u8 (the --save-image export of `python -m adaptiveisp_amd.val`) at 8 x 720 x 1280 against the copy
ceiling: the event-timed mean per launch, and a device-to-device copy of the same fp32 input bytes timed the same way
(read + write of 4 B/sample), scaled to the export's bytes (4 B/sample read + 1 B/sample written). Inputs rotate over
`--bufs` batches so that the working set exceeds the 256 MB last-level cache. One JSON line.
    python tools/export_bench.py [--reps 200] [--B 8] [--H 720] [--W 1280] [--bufs 4]"""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from adaptiveisp_amd import _lib  # noqa: E402


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
    ap.add_argument("--reps", type=int, default=200)
    ap.add_argument("--B", type=int, default=8)
    ap.add_argument("--H", type=int, default=720)
    ap.add_argument("--W", type=int, default=1280)
    ap.add_argument("--bufs", type=int, default=4)
    a = ap.parse_args()
    g = torch.Generator(device="cuda").manual_seed(0)
    ins = [torch.rand(a.B, 3, a.H, a.W, device="cuda", generator=g) * 1.2 - 0.1 for _ in range(a.bufs)]
    outs = [torch.empty(a.B, a.H, a.W, 3, dtype=torch.uint8, device="cuda") for _ in range(a.bufs)]
    copies = [torch.empty_like(ins[0]) for _ in range(a.bufs)]
    export_us = _time(lambda i: _lib.export_u8(ins[i % a.bufs], out=outs[i % a.bufs]), a.reps)
    copy_us = _time(lambda i: copies[i % a.bufs].copy_(ins[(i + 1) % a.bufs]), a.reps)
    n = a.B * 3 * a.H * a.W
    copy_bytes, export_bytes = 8 * n, 5 * n
    copy_rate = copy_bytes / (copy_us * 1e-6)
    print(json.dumps({"B": a.B, "H": a.H, "W": a.W, "export_us": round(export_us, 2), "export_bytes": export_bytes,
                      "export_TBps": round(export_bytes / (export_us * 1e-6) / 1e12, 2), "copy_us": round(copy_us, 2),
                      "copy_TBps": round(copy_rate / 1e12, 2),
                      "copy_ceiling_us": round(export_bytes / copy_rate * 1e6, 2),
                      "export_over_ceiling": round(export_us / (export_bytes / copy_rate * 1e6), 3)}))


if __name__ == "__main__":
    main()
