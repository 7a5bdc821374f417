#!/usr/bin/env python3
"""Interleaved A/B in ONE process of the tuned detector forward at the benchmark's size between the MFMA shapes of the two ring
kernel families (adayolo_set_mfma_shape; settings "PP,PP128", e.g. 32,32 16,16 16,32 32,16): one engine per setting, its
forward captured into a hipGraph while the setting holds (a graph keeps the kernels it captured), `rounds` x `reps` replays
interleaved on random data; prediction differences are printed. --per-layer: every launch of the 256 x 256 / 256 x 128 kernels
(and the chains) of the plan alone, back to back under each setting (event pairs, median of 9), so that the layers a shape
wins or loses can be read off.
usage (GPU box): python tools/mfma_shape_ab.py 32,32 16,16 16,32 32,16 [--rounds 10] [--per-layer]"""
import argparse
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("settings", nargs="+")
    ap.add_argument("--rounds", type=int, default=10)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--height", type=int, default=720)
    ap.add_argument("--width", type=int, default=1280)
    ap.add_argument("--per-layer", action="store_true")
    a = ap.parse_args()
    from _synth import synth_yolo_state_dict, test_image
    from adaptiveisp_amd.yolo import YoloEngine, _lib, yolov3
    L = _lib.load()
    dev = torch.device("cuda:0")
    tune = os.path.join(ROOT, "adaptiveisp_amd", "yolo", "tuning", "mi355x.json")
    det = yolov3()
    det.load_state_dict(synth_yolo_state_dict(det, seed=2))
    det = det.eval()
    x = torch.from_numpy(test_image(a.batch, a.height, a.width, seed=3, special=False)).to(dev)
    default = (L.adayolo_get_mfma_shape(0), L.adayolo_get_mfma_shape(1))
    print(f"library default: pp {default[0]}, pp128 {default[1]}")

    def select(s):
        pp, pp128 = (int(v) for v in s.split(","))
        assert L.adayolo_set_mfma_shape(0, pp) == 0 and L.adayolo_set_mfma_shape(1, pp128) == 0

    engines, graphs, preds = {}, {}, {}
    for s in a.settings:
        select(s)
        e = YoloEngine(det, a.batch, a.height, a.width, device=dev)
        e.autotune(cache=tune, write=False)
        engines[s] = e
        preds[s] = e(x).clone()
        torch.cuda.synchronize()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
            e(x)
        graphs[s] = g
    base = a.settings[0]
    for s in a.settings[1:]:
        d = (preds[s] - preds[base]).abs()
        print(f"[{s}] vs [{base}]: max |d| {d.max().item():.3e} (max |pred| {preds[base].abs().max().item():.1f})")
    times = {s: [] for s in a.settings}
    for r in range(a.rounds):
        order = a.settings if r % 2 == 0 else list(reversed(a.settings))
        for s in order:
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            graphs[s].replay()
            e0.record()
            for _ in range(a.reps):
                graphs[s].replay()
            e1.record()
            torch.cuda.synchronize()
            times[s].append(e0.elapsed_time(e1) / a.reps)
    for s in a.settings:
        t = times[s]
        print(f"detector forward [{s}]: median {statistics.median(t):.4f} ms  min {min(t):.4f}  max {max(t):.4f}   "
              f"/ [{base}] = {statistics.median(t) / statistics.median(times[base]):.4f}", flush=True)
    if a.per_layer:
        st = _lib.stream_ptr()
        e = engines[base]
        rows = {}
        for kind, fn, args in e.plan:
            if kind == "conv" and args[16] in (50, 60):
                key = f"conv {args[9]}x{args[10]} {args[11]}->{args[12]} k{args[13]}s{args[14]} v{args[16]}"
            elif kind == "conv2":
                key = f"conv2 {args[9]}x{args[10]} {args[11]}->{args[12]} k{args[13]}s{args[14]} fused"
            elif kind == "chain":
                key = f"chain of {args[1]} layers"
            else:
                continue
            for s in a.settings:
                select(s)
                ts = []
                for _ in range(9):
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    e0.record()
                    fn(*args, st)
                    e1.record()
                    e1.synchronize()
                    ts.append(e0.elapsed_time(e1) * 1e3)
                r_ = rows.setdefault(key, {}).setdefault(s, [0, 0.0])
                r_[0] += 1
                r_[1] += statistics.median(ts)
        print("--- per launch alone (median of 9), us each: " + "  ".join(f"[{s}]" for s in a.settings))
        for key, by in rows.items():
            n = by[base][0]
            print(f"  x{n:2d} " + "  ".join(f"{by[s][1] / n:8.1f}" for s in a.settings) + f"   {key}")
        for s in a.settings:
            print(f"  sum [{s}] {sum(by[s][1] for by in rows.values()):.1f} us")
    select(f"{default[0]},{default[1]}")


if __name__ == "__main__":
    main()
