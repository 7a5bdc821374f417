#!/usr/bin/env python3
"""adaisp_resize_u8 (ImageFolderSource(resize="device")) at 8 sources of one size -> 512 on the long side, for 640 x 480,
1280 x 720 and 4032 x 3024 (load_image's general area filter at every one), against the copy ceiling: a device-to-device
copy of the source bytes, launched the same way. Sources rotate over `--bufs` batches so that the working set of the large
size exceeds the last-level cache. Kernel times come from `rocprofv3 --kernel-trace --stats`: with --profile the tool runs
itself under it in a child process and reads the stats (k_resize_u8 and the copy kernel); without it, event-timed means.
One JSON line per size.
    python tools/resize_bench.py [--profile] [--reps 100] [--B 8] [--S 512] [--bufs 4]"""
import argparse
import csv
import glob
import json
import math
import os
import subprocess
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIZES = [(480, 640), (720, 1280), (3024, 4032)]


def _child(a):
    import torch
    sys.path.insert(0, ROOT)
    from adaptiveisp_amd import _lib
    from adaptiveisp_amd.resize import TapPlan
    rs = np.random.RandomState(0)
    H, W = a.src
    r = a.S / max(H, W)
    h, w = math.ceil(H * r), math.ceil(W * r)
    plan = TapPlan()
    for b in range(a.B):
        plan.add((H, W), (h, w), True, b * H * W * 3, b * h * w * 3)
    rec = plan.descriptors()
    desc = torch.from_numpy(rec.view(np.uint8).copy()).cuda()
    tabs = torch.from_numpy(plan.table().copy()).cuda()
    srcs = [torch.from_numpy(rs.randint(0, 256, a.B * H * W * 3).astype(np.uint8)).cuda() for _ in range(a.bufs)]
    dsts = [torch.empty(a.B * h * w * 3, dtype=torch.uint8, device="cuda") for _ in range(a.bufs)]
    copies = [torch.empty_like(srcs[0]) for _ in range(a.bufs)]

    def timed(fn):
        for i in range(5):
            fn(i)
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for i in range(a.reps):
            fn(i)
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) / a.reps * 1e3
    rus = timed(lambda i: _lib.resize_u8(srcs[i % a.bufs], dsts[i % a.bufs], desc, tabs, rec))
    cus = timed(lambda i: copies[i % a.bufs].copy_(srcs[(i + 1) % a.bufs]))
    print("RESULT " + json.dumps(dict(src_hw=[H, W], dst_hw=[h, w], read_bytes=a.B * H * W * 3,
                                      write_bytes=a.B * h * w * 3, event_resize_us=round(rus, 2),
                                      event_copy_us=round(cus, 2))), flush=True)


def _stats(outdir):
    """kernel name -> (calls, mean ns) from the rocprofv3 stats CSV(s) under outdir."""
    out = {}
    for f in glob.glob(os.path.join(outdir, "**", "*kernel_stats.csv"), recursive=True):
        for row in csv.DictReader(open(f)):
            out[row["Name"]] = (int(row["Calls"]), float(row["AverageNs"]))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--profile", action="store_true", help="kernel times from rocprofv3 --kernel-trace --stats")
    ap.add_argument("--reps", type=int, default=100)
    ap.add_argument("--B", type=int, default=8)
    ap.add_argument("--S", type=int, default=512)
    ap.add_argument("--bufs", type=int, default=4)
    ap.add_argument("--timeout", type=int, default=300, help="seconds per child")
    ap.add_argument("--src", type=int, nargs=2, default=None, help=argparse.SUPPRESS)   # the child: one source size
    a = ap.parse_args()
    if a.src:
        return _child(a)
    for H, W in SIZES:
        args = ["--reps", str(a.reps), "--B", str(a.B), "--S", str(a.S), "--bufs", str(a.bufs), "--src", str(H), str(W)]
        with tempfile.TemporaryDirectory() as tmp:
            cmd = [sys.executable, os.path.abspath(__file__)] + args
            if a.profile:
                cmd = ["rocprofv3", "--kernel-trace", "--stats", "-f", "csv", "-d", tmp, "-o", "resize", "--"] + cmd
            p = subprocess.run(["timeout", "-k", "10", str(a.timeout)] + cmd, cwd=ROOT, capture_output=True, text=True)
            if p.returncode != 0:
                print(json.dumps({"src_hw": [H, W], "returncode": p.returncode, "stderr": p.stderr[-3000:]}), flush=True)
                raise SystemExit(p.returncode)
            r = json.loads([ln for ln in p.stdout.splitlines() if ln.startswith("RESULT ")][-1][7:])
            stats = _stats(tmp) if a.profile else {}
        nbytes = r["read_bytes"] + r["write_bytes"]
        resize_us, copy_us = r["event_resize_us"], r["event_copy_us"]
        for name, (calls, ns) in stats.items():
            if "k_resize_u8" in name:
                resize_us, r["kernel_resize_calls"] = ns / 1e3, calls
            elif "opy" in name:
                copy_us, r["kernel_copy_name"] = ns / 1e3, name[:60]
        r["timing"] = "rocprofv3 kernel" if "kernel_resize_calls" in r else "events"
        r["copy_timing"] = "rocprofv3 kernel" if "kernel_copy_name" in r else "events"
        copy_rate = 2 * r["read_bytes"] / (copy_us * 1e-6)           # the copy reads and writes the source bytes
        r.update(resize_us=round(resize_us, 2), copy_us=round(copy_us, 2),
                 resize_GBps=round(nbytes / (resize_us * 1e-6) / 1e9, 1), copy_GBps=round(copy_rate / 1e9, 1),
                 copy_ceiling_us=round(nbytes / copy_rate * 1e6, 2),
                 over_ceiling=round(resize_us / (nbytes / copy_rate * 1e6), 2))
        print(json.dumps(r), flush=True)


if __name__ == "__main__":
    main()
