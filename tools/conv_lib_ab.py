#!/usr/bin/env python3
"""The ring conv kernels between builds of libadayolo.so in ONE process: the same seeded inputs through every library, every
output array compared in bits with the in-tree build's, a median time per entry and library (interleaved rounds).
Entries: adayolo_conv_fwd_variant for every engine.TUNE_CANDIDATES variant (split-K through its own entry point), the fused 1x1,
a mixed-tile chain, keep, dsilu and s2grad — under both MFMA shapes, at a ragged small shape and a baseline layer shape.
usage (GPU box): python tools/conv_lib_ab.py name=path/to/libadayolo.so [...]      exit code 1: some output differs"""
import ctypes
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from adaptiveisp_amd.yolo import _lib, engine  # noqa: E402

DEV = "cuda:0"
vp = ctypes.c_void_p

libs = {"in-tree": _lib.load()}
for a in sys.argv[1:]:
    n, p = a.split("=")
    libs[n] = _lib.load(os.path.abspath(p))
st = _lib.stream_ptr()
P = lambda t: vp(t.data_ptr()) if t is not None else None  # noqa: E731
nan = lambda *s: torch.full(s, float("nan"), dtype=torch.bfloat16, device=DEV)  # noqa: E731
totals = {"entries": 0, "arrays": 0, "different": 0, "not served": 0}


def operands(B, H, W, cin, cout, k, seed):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(B, H, W, cin, generator=g).to(torch.bfloat16).to(DEV)
    w = (torch.randn(cout, k, k, cin, generator=g) / (k * k * cin) ** 0.5).to(torch.bfloat16).to(DEV)
    b = torch.randn(cout, generator=g).to(DEV)
    return g, x, w, b


def entry(label, make):
    """make(L) -> (launch, outputs) or None where the library does not serve the case; launch() returns the C return code"""
    got, times = {}, {n: [] for n in libs}
    for n, L in libs.items():
        got[n] = make(L)
    if any(v is None for v in got.values()):
        assert all(v is None for v in got.values()), (label, "served by one build only")
        totals["not served"] += 1
        return
    for rnd in range(5):
        for n in libs:
            launch = got[n][0]
            assert launch() == 0, (label, n)
            torch.cuda.synchronize()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(5):
                launch()
            e1.record()
            torch.cuda.synchronize()
            times[n].append(e0.elapsed_time(e1) / 5 * 1e3)
    ref = got["in-tree"][1]
    bad = []
    for n in libs:
        for i, (o, r) in enumerate(zip(got[n][1], ref)):
            totals["arrays"] += n != "in-tree"
            if n != "in-tree" and not torch.equal(o.view(torch.int16), r.view(torch.int16)):
                bad.append(f"{n}[{i}]")
    assert not any(torch.isnan(r.float()).any() for r in ref), (label, "unwritten output")
    totals["entries"] += 1
    totals["different"] += len(bad)
    print(f"{label}: " + "  ".join(f"{n} {statistics.median(v):.1f} us" for n, v in times.items()) +
          (f"  DIFFERS: {' '.join(bad)}" if bad else "  bits equal"), flush=True)


def conv_case(v, shape, seed):
    B, H, W, cin, cout, k, use_res = shape
    g, x, w, b = operands(B, H, W, cin, cout, k, seed)
    res = torch.randn(B, H, W, cout, generator=g).to(torch.bfloat16).to(DEV) if use_res else None

    def make(L):
        out = nan(B, H, W, cout)
        common = (P(x), cin, P(w), P(b), P(res), cout if use_res else 0, P(out), cout)
        if v >= engine.SPLITK_BASE:
            nws = int(L.adayolo_conv_splitk_workspace_bytes(B, H, W, cin, cout, k, 1, v))
            if nws == 0:
                return None
            ws = torch.zeros(nws, dtype=torch.uint8, device=DEV)
            fn = lambda: L.adayolo_conv_splitk_fwd(*common, None, 0, B, H, W, cin, cout, k, 1, 1, v, P(ws), nws, st)  # noqa: E731
        else:
            if not engine.serves(v, (B, H, W, cin, cout, k, 1, 1)):
                return None
            fn = lambda: L.adayolo_conv_fwd_variant(*common, B, H, W, cin, cout, k, 1, 1, v, st)  # noqa: E731
        return (fn, [out]) if fn() == 0 else None
    entry(f"variant {v} {shape}", make)


def keep_dsilu_case(v, shape, seed):
    B, H, W, cin, cout, k, use_res = shape
    g, x, w, b = operands(B, H, W, cin, cout, k, seed)
    res = torch.randn(B, H, W, cout, generator=g).to(torch.bfloat16).to(DEV) if use_res else None
    pre_in = (torch.randn(B, H, W, cout, generator=g) * 2).to(torch.bfloat16).to(DEV)

    def ws_of(L):
        if v < engine.SPLITK_BASE:
            return None, 0
        nws = int(L.adayolo_conv_splitk_workspace_bytes(B, H, W, cin, cout, k, 1, v))
        return (torch.zeros(nws, dtype=torch.uint8, device=DEV) if nws else None), nws

    def keep(L):
        ws, nws = ws_of(L)
        if v >= engine.SPLITK_BASE and not nws:
            return None
        out, pre = nan(B, H, W, cout), nan(B, H, W, cout)
        common = (P(x), cin, P(w), P(b), P(res), cout if use_res else 0, P(out), cout, P(pre), cout, B, H, W, cin, cout, k, 1, 1, v)
        fn = (lambda: L.adayolo_conv_splitk_fwd(*common, P(ws), nws, st)) if ws is not None else (lambda: L.adayolo_conv_keep_fwd(*common, st))
        return (fn, [out, pre]) if fn() == 0 else None

    def dsilu(L):
        ws, nws = ws_of(L)
        if v >= engine.SPLITK_BASE and not nws:
            return None
        gy, gp = nan(B, H, W, cout), nan(B, H, W, cout)
        fn = lambda: L.adayolo_conv_dsilu_fwd(P(x), cin, P(w), P(b), P(res), cout if use_res else 0, P(gy), cout, P(pre_in), cout,  # noqa: E731
                                              P(gp), cout, B, H, W, cin, cout, k, 1, v, P(ws), nws, st)
        return (fn, [gy, gp]) if fn() == 0 else None
    entry(f"keep {v} {shape}", keep)
    entry(f"dsilu {v} {shape}", dsilu)


def s2grad_case(v, shape, seed):
    B, Ho, Wo, cin, cout, use_res = shape                 # the stride-2 conv cin -> cout whose data gradient this is
    g = torch.Generator().manual_seed(seed)
    gy = torch.randn(B, Ho, Wo, cout, generator=g).to(torch.bfloat16).to(DEV)
    w4 = (torch.randn(4 * cin, 2, 2, cout, generator=g) / (4 * cout) ** 0.5).to(torch.bfloat16).to(DEV)
    zb = torch.zeros(4 * cin, device=DEV)
    res = torch.randn(B, 2 * Ho, 2 * Wo, cin, generator=g).to(torch.bfloat16).to(DEV) if use_res else None
    pre = (torch.randn(B, 2 * Ho, 2 * Wo, cin, generator=g) * 2).to(torch.bfloat16).to(DEV)

    def make(L):
        ws, nws = None, 0
        if v >= engine.SPLITK_BASE:
            nws = int(L.adayolo_conv_splitk_workspace_bytes(B, Ho, Wo, cout, 4 * cin, 2, 1, v))
            if nws == 0:
                return None
            ws = torch.zeros(nws, dtype=torch.uint8, device=DEV)
        gx, gp = nan(B, 2 * Ho, 2 * Wo, cin), nan(B, 2 * Ho, 2 * Wo, cin)
        fn = lambda: L.adayolo_conv_s2grad_fwd(P(gy), cout, P(w4), P(zb), P(res), cin if use_res else 0, P(gx), cin, P(pre), cin,  # noqa: E731
                                               P(gp), cin, B, Ho, Wo, cout, cin, v, P(ws), nws, st)
        return (fn, [gx, gp]) if fn() == 0 else None
    entry(f"s2grad {v} {shape}", make)


def fused_case(shape, seed):
    B, H, W, cin, k, use_res = shape
    g, x, w, b = operands(B, H, W, cin, 256, k, seed)
    res = torch.randn(B, H, W, 256, generator=g).to(torch.bfloat16).to(DEV) if use_res else None
    w2 = (torch.randn(128, 256, generator=g) / 16).to(torch.bfloat16).to(DEV)
    w2p = w2.reshape(4, 32, 16, 2, 8).permute(0, 2, 3, 1, 4).contiguous()      # fragment-major (include/adayolo.h)
    b2 = torch.randn(128, generator=g).to(DEV)

    def make(L):
        out, out2 = nan(B, H, W, 256), nan(B, H, W, 128)
        fn = lambda: L.adayolo_conv_fused1x1_fwd(P(x), cin, P(w), P(b), P(res), 256 if use_res else 0, P(out), 256, B, H, W, cin, 256,  # noqa: E731
                                                 k, 1, 1, P(w2p), P(b2), P(out2), 128, 128, st)
        return (fn, [out, out2]) if fn() == 0 else None
    entry(f"fused1x1 {shape}", make)


def chain_case(shape, seed):
    """x -> 3x3 256 -> 256 (256 x 256 tile, the next 1x1 fused: out, out2) -> 3x3 128 -> 256 + out as residual (256 x 128 tile)"""
    B, H, W = shape
    g, x, w0, b0 = operands(B, H, W, 256, 256, 3, seed)
    w2 = (torch.randn(128, 256, generator=g) / 16).to(torch.bfloat16).to(DEV)
    w2p = w2.reshape(4, 32, 16, 2, 8).permute(0, 2, 3, 1, 4).contiguous()
    b2 = torch.randn(128, generator=g).to(DEV)
    w1 = (torch.randn(256, 3, 3, 128, generator=g) / (9 * 128) ** 0.5).to(torch.bfloat16).to(DEV)
    b1 = torch.randn(256, generator=g).to(DEV)

    def make(L):
        y0, h, y1 = nan(B, H, W, 256), nan(B, H, W, 128), nan(B, H, W, 256)
        arr = (_lib.ChainLayer * 2)()
        for c, (i, ic, wt, bs, r, o, cin, tile) in zip(arr, ((x, 256, w0, b0, None, y0, 256, 0), (h, 128, w1, b1, y0, y1, 128, 1))):
            c.in_, c.in_cstride, c.weight, c.bias = i.data_ptr(), ic, wt.data_ptr(), bs.data_ptr()
            c.residual, c.res_cstride = (r.data_ptr(), 256) if r is not None else (None, 0)
            c.out, c.out_cstride = o.data_ptr(), 256
            c.B, c.H, c.W, c.Cin, c.Cout, c.ksize, c.stride, c.act, c.tile = B, H, W, cin, 256, 3, 1, _lib.ACT_SILU, tile
        arr[0].weight2, arr[0].bias2, arr[0].out2, arr[0].out2_cstride, arr[0].Cout2 = w2p.data_ptr(), b2.data_ptr(), h.data_ptr(), 128, 128
        nbytes = int(L.adayolo_conv_chain_workspace_bytes(arr, 2))
        if nbytes <= 0:
            return None
        ws = torch.empty((nbytes,), dtype=torch.uint8, device=DEV)
        if L.adayolo_conv_chain_prepare(arr, 2, P(ws), nbytes) != 0:
            return None
        fn = lambda: L.adayolo_conv_chain_fwd(arr, 2, P(ws), nbytes, st)  # noqa: E731
        fn.keep = (arr, ws)
        return (fn, [y0, h, y1]) if fn() == 0 else None
    entry(f"chain (256x256 fused | 256x128) {shape}", make)


SMALL = (1, 9, 7, 256, 256, 3, True)                       # M = 63: one ragged tile; 3 x 3: nK odd per tap
BASE = {2: (8, 46, 80, 64, 64, 3, False), 5: (8, 46, 80, 128, 128, 3, True), 22: (8, 92, 160, 64, 64, 1, False),
        26: (8, 46, 80, 128, 256, 1, False), 27: (8, 46, 80, 256, 128, 1, False), 40: (8, 92, 160, 64, 64, 3, False),
        50: (8, 46, 80, 256, 256, 3, True), 60: (8, 23, 40, 512, 512, 3, True), 80: (8, 46, 80, 128, 128, 3, True),
        85: (8, 23, 40, 256, 128, 1, False), 90: (8, 92, 160, 64, 64, 3, True)}
for ms in (32, 16):
    for L in libs.values():
        assert L.adayolo_set_mfma_shape(0, ms) == 0 and L.adayolo_set_mfma_shape(1, ms) == 0
    print(f"---- MFMA shape {ms}", flush=True)
    for v in engine.TUNE_CANDIDATES:
        if v >= engine.SPLITK_BASE:
            conv_case(v, (2, 13, 17, 256, 128, 3, True), 300 + v)
            conv_case(v, (8, 16, 16, 1024, 512, 3, True), 400 + v)
        else:
            conv_case(v, SMALL if v not in (2, 22, 40, 90) else (1, 9, 7, 64, 64, 3, v == 90), 100 + v)
            conv_case(v, BASE[v], 200 + v)
    fused_case((1, 9, 7, 256, 3, True), 1)
    fused_case((8, 46, 80, 256, 3, True), 2)
    chain_case((1, 19, 17), 3)
    chain_case((8, 46, 80), 4)
    for v in (60, 80, engine.SPLITK_BASE + 4):
        keep_dsilu_case(v, (2, 13, 17, 256, 128, 3, True), 500 + v)
        keep_dsilu_case(v, (8, 16, 16, 1024, 512, 3, True), 600 + v)
    for v in (60, engine.SPLITK_BASE + 4):
        s2grad_case(v, (1, 5, 7, 32, 64, True), 700 + v)
        s2grad_case(v, (8, 16, 16, 512, 1024, True), 800 + v)
print("totals: " + ", ".join(f"{k} {v}" for k, v in totals.items()), flush=True)
sys.exit(1 if totals["different"] else 0)
