#!/usr/bin/env python3
"""adaisp_unprocess at the trainer's refill size (8 x 512 x 512 from 512 x 384 sources, the letterbox of a 4:3 photo):
convert, unprocess and unprocess + noise, each launched back to back; prints the event-timed mean per launch and the bytes
and bound. Kernel times: run it under `rocprofv3 --kernel-trace --stats -d OUT -o run -- python tools/unprocess_bench.py`.
    python tools/unprocess_bench.py [--reps 200] [--B 8] [--S 512]"""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from adaptiveisp_amd import _lib  # noqa: E402
from adaptiveisp_amd.data import kernel_params, sample_unprocess_params  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=200)
    ap.add_argument("--B", type=int, default=8)
    ap.add_argument("--S", type=int, default=512)
    a = ap.parse_args()
    B, S = a.B, a.S
    h, w = S * 3 // 4, S
    rs = np.random.RandomState(0)
    src = torch.from_numpy(rs.randint(0, 256, size=B * h * w * 3).astype(np.uint8)).cuda()
    desc = np.zeros(B, _lib.UNPROCESS_DESC)
    for b in range(B):
        desc[b]["src_offset"], desc[b]["h"], desc[b]["w"], desc[b]["top"], desc[b]["serial"] = b * h * w * 3, h, w, (S - h) // 2, b
        desc[b]["p"] = kernel_params(sample_unprocess_params(rs, True, (0.1, 0.3)))
    d = torch.from_numpy(desc.view(np.uint8).copy()).cuda()
    out = torch.empty(B, 3, S, S, device="cuda")
    res = {}
    for name, flags in (("convert", 0), ("unprocess", _lib.UNP_UNPROCESS), ("noise", _lib.UNP_UNPROCESS | _lib.UNP_NOISE)):
        for _ in range(10):
            _lib.unprocess(src, d, S, seed=1, flags=flags, out=out)
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(a.reps):
            _lib.unprocess(src, d, S, seed=1, flags=flags, out=out)
        e1.record()
        torch.cuda.synchronize()
        res[name] = round(e0.elapsed_time(e1) / a.reps * 1e3, 2)
    nbytes = B * h * w * 3 + B * 3 * S * S * 4
    print(json.dumps({"B": B, "S": S, "src_hw": [h, w], "us_per_launch": res, "bytes": nbytes,
                      "copy_bound_us_at_5TBps": round(nbytes / 5e12 * 1e6, 2)}))


if __name__ == "__main__":
    main()
