#!/usr/bin/env python3
"""Image backward (adaisp_backward_image) per op at 8 x 720 x 1280: device-event time of one call, the achieved bytes/s
against the 36 B/px streaming roof (read img + grad_out, write grad_img), and the forward of the same op for scale.
Event times include the launches that return at once for the other families; kernel times come from a separate
`rocprofv3 --kernel-trace --stats` run of this script.

    python tools/imggrad_bench.py [--iters N] [--ops E,G,...] [--batch B]
"""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from adaptiveisp_amd import _lib  # noqa: E402

NAMES = ("E", "G", "CCM", "Shr", "NLM", "T", "Ct", "Sp", "BW", "W", "USM", "ShrV2", "C")
ROOF_BPS = 6.2e12          # non-temporal float4 copy ceiling (tools/stream_ceiling.hip)


def timed(fn, iters):
    fn()
    torch.cuda.synchronize()
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
    ev[0].record()
    for _ in range(iters):
        fn()
    ev[1].record()
    torch.cuda.synchronize()
    return ev[0].elapsed_time(ev[1]) / iters * 1e3        # us per call


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--ops", default=",".join(NAMES))
    ap.add_argument("--batch", type=int, default=8)
    a = ap.parse_args()
    B, H, W = a.batch, 720, 1280
    g = torch.Generator(device="cpu").manual_seed(1234)
    x = (torch.rand(B, 3, H, W, generator=g) ** 2.2 * 0.5).cuda()
    go = torch.randn(B, 3, H, W, generator=g).cuda()
    p = torch.rand(B, _lib.MAX_PARAMS, generator=g).cuda() * 0.8 + 0.6
    nbytes = 36.0 * B * H * W
    for name in a.ops.split(","):
        op = NAMES.index(name)
        ids = torch.full((B,), op, dtype=torch.int32, device="cuda")
        t_bwd = timed(lambda: _lib.backward_image(x, go, ids, p, clip=True), a.iters)
        t_fwd = timed(lambda: _lib.forward(x, ids, p, clip=True), a.iters)
        print(json.dumps({"op": name, "B": B, "H": H, "W": W, "bwd_image_us": round(t_bwd, 1), "fwd_us": round(t_fwd, 1),
                          "bwd_TBps_at_36Bpx": round(nbytes / t_bwd / 1e6, 3),
                          "roof_fraction": round(nbytes / t_bwd / 1e6 / (ROOF_BPS / 1e12), 3)}), flush=True)


if __name__ == "__main__":
    main()
